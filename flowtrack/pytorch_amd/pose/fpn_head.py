"""The FPN top-down head (pose_fpn.py:48-104) as a mixin of a host.PoseHost subclass whose trunk leaves its four stage maps in
stages["layer1"] .. ["layer3"] and `cur`: resnet_models.FpnResnet and densenet.FpnDensenet."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..hip_ops import ActView, fold_scale_shift, new_act, record_upsample_ac
from ..params import ActMarker, BatchNormParams, ConvParams


def _bn_relu_conv(cin: int, cout: int, kernel_size: int, padding: int = 0, bias: bool = True) -> nn.Sequential:
    """_make_conv of pose_fpn.py:41-46: BatchNorm, ReLU, conv — pre-activation order, so index 0 is the BN and 2 the conv."""
    return nn.Sequential(BatchNormParams(cin), ActMarker("relu"), ConvParams(cin, cout, kernel_size, padding=padding, bias=bias))


class FpnHead:
    """FPN top-down path + 1x1 heatmap conv.  With c2..c5 the maps behind the trunk's four stages:

        p5 = latlayer1(c5)
        p4 = toplayer1(up(p5) + latlayer2(c4)),  p3 = toplayer2(up(p4) + latlayer3(c3)),  p2 = toplayer3(up(p3) + latlayer4(c2))
        heatmaps = heatmap(p2)                      toplayer_j, heatmap = BatchNorm -> ReLU -> conv;  up = bilinear, align_corners=True

    Each top-down step is three launches.  With (s, b) the fold of toplayer_j's BatchNorm,
    relu(bn(up(p) + lat(c))) = relu(s * lat(c) + b + s * up(p)): ft_upsample_bilinear_ac_fwd writes u = s * up(p), the lateral 1x1 conv
    takes s, b as its scale / shift and u as its residual input, and toplayer_j's 3x3 conv reads the activated map (its zero padding
    pads that map, as in the reference).  Nothing else reads the un-normalised sum.  The last 3x3 conv carries heatmap.0's BatchNorm
    and ReLU in its epilogue, since only the heatmap conv reads p2."""

    def _make_head(self, num_classes: int, planes=(2048, 1024, 512, 256)) -> None:
        """`planes`: the channels of c5, c4, c3, c2."""
        feats = 256
        for i, cin in enumerate(planes, start=1):                       # lateral layers (pose_fpn.py:54-58): latlayer1 reads c5
            setattr(self, f"latlayer{i}", ConvParams(cin, feats, 1, bias=False))
        for j in (1, 2, 3):                                             # top-down layers (pose_fpn.py:60-63)
            setattr(self, f"toplayer{j}", _bn_relu_conv(feats, feats, 3, padding=1, bias=False))
        self.heatmap = _bn_relu_conv(feats, num_classes, 1)

    def _init_head(self) -> None:
        # pose_fpn.py:92-104
        for name, m in self.named_modules():
            if "lat" in name or "top" in name:
                if isinstance(m, ConvParams):
                    nn.init.normal_(m.weight, std=0.001)
                elif isinstance(m, BatchNormParams):
                    nn.init.constant_(m.weight, 1)
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.heatmap[2].weight, std=0.001)
        nn.init.constant_(self.heatmap[2].bias, 0)

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        B, mk = cur.N, dict(dtype=dtype, device=device)
        feats = self.latlayer1.cout
        p = new_act(B, cur.H, cur.W, feats, dtype, device)
        self._record_p5(prog, cur, p, dtype, device)
        stages["p5"] = p
        for j, stage in ((1, "layer3"), (2, "layer2"), (3, "layer1")):
            lat, top, c = getattr(self, f"latlayer{j + 1}"), getattr(self, f"toplayer{j}"), stages[stage]
            bn = top[0].as_dict()
            scale = self._cached(f"toplayer{j}.0.scale", dtype, device, lambda: fold_scale_shift(feats, feats, None, bn, device)[0])
            u = new_act(B, c.H, c.W, feats, dtype, device)
            record_upsample_ac(prog, p, u, scale)
            a = new_act(B, c.H, c.W, feats, dtype, device)
            self.fused(f"latlayer{j + 1}+toplayer{j}.0", lat.weight, bn=bn, act="relu", **mk).record(prog, c, a, residual=u)
            last = j == 3
            conv = self.fused(f"toplayer{j}.2" + ("+heatmap.0" if last else ""), top[2].weight, pad=1,
                              bn=self.heatmap[0].as_dict() if last else None, act="relu" if last else None, **mk)
            p = new_act(B, c.H, c.W, feats, dtype, device)
            conv.record(prog, a, p)
            stages[f"p{5 - j}"] = p
        heatmaps = torch.empty((B, self.num_classes, p.H, p.W), dtype=torch.float32, device=device)
        self.fused("heatmap.2", self.heatmap[2].weight, bias=self.heatmap[2].bias, act=None, **mk).record(prog, p, heatmaps)
        return heatmaps

    def _record_p5(self, prog, cur: ActView, p: ActView, dtype, device) -> None:
        """p5 = latlayer1(c5) from the trunk's last map `cur` (here c5 itself)."""
        self.fused("latlayer1", self.latlayer1.weight, act=None, dtype=dtype, device=device).record(prog, cur, p)
