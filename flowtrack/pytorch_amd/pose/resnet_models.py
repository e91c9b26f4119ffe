"""The pose models on a ResNet-50/101/152 trunk: PoseResnet (the trunk and its recording on host.PoseHost) and its three heads,
DeconvResnet (pose_deconv.py), FpnResnet (pose_fpn.py) and LateralDeconvResnet (pose_net.py)."""
from __future__ import annotations

import os
from typing import List

import torch
import torch.nn as nn

from ..hip_ops import (ActView, FlowtrackHipError, FusedConv, FusedLateralDeconv, record_scale_shift_act, bottleneck_exit_fusable, new_act,
                       record_bottleneck_exit, fold_scale_shift)
from ..params import ActMarker, BatchNormParams, ConvParams, ConvTransposeParams
from ..resnet import Bottleneck, record_block
from .fpn_head import FpnHead, _bn_relu_conv
from .host import PoseHost, PooledStem, _Stages


class PoseResnet(PooledStem, PoseHost):
    """The ResNet trunk and its recording.  A model adds its head through three hooks: _make_head (parameters, under the
    reference's names), _init_head (the reference's init_net) and _record_head (the launches from the stage maps to the NCHW fp32
    heat maps)."""
    #: True: the head reads the full maps of layer1..layer3 as well as layer4's, so every stage seam is recorded as today's
    #: launches whatever fuse_stage_exit says (the exit form writes only the even pixels of a stage's last block), and
    #: split_lanes stays off
    full_stage_maps: bool = False
    #: fold each block-0 projection shortcut into its conv3 launch (FusedShortcutConv); FT_FUSE_SHORTCUT=0 keeps them apart
    fuse_shortcut: bool = os.environ.get("FT_FUSE_SHORTCUT", "1") != "0"
    #: identity-shortcut blocks of the 256-wide stage as one launch (ft_bottleneck_fwd); FT_FUSE_BOTTLENECK=0 keeps 3 convs
    fuse_bottleneck: bool = os.environ.get("FT_FUSE_BOTTLENECK", "1") != "0"
    #: a stage's last identity block together with the next stage's conv1 as one launch that writes t1 and only the even pixels of
    #: the block's output (ft_bottleneck_exit_fwd; layer1.2 + layer2.0.conv1): recorded as an alternative to today's launches, the
    #: first-call benchmark keeps one.  FT_FUSE_STAGE_EXIT=0 / False records today's launches only, 2 / "force" the exit form only (dev, tests)
    fuse_stage_exit = {"0": False, "2": "force"}.get(os.environ.get("FT_FUSE_STAGE_EXIT", "1"), True)
    #: dev: layer1 + layer2 as two half-batch lanes (parallel graph branches); FT_SPLIT_LANES=1
    split_lanes4: bool = os.environ.get("FT_SPLIT_LANES4", "0") == "1"       # dev: layer4 as two half-batch lanes
    split_lanes: int = int(os.environ.get("FT_SPLIT_LANES", "0") or 0)     # 1: lanes start together; 2: the second lane starts with its half of the stem
    #: offer the cluster form of the 256-plane identity blocks (ft_bottleneck_cluster_fwd) to the first-call benchmark
    #: (FT_CLUSTER_KERNELS=1).  OFF by default: measured in situ at R50 batch 64 it takes 50-52 us per block against the strip
    #: form's 48 (each of its two in-launch hand-offs costs 4-5 us: profiles/README.md, round 5), and its workgroups wait for
    #: each other inside the launch (bounded spins: nothing deadlocks, but a timed-out hand-off gives a wrong block).
    cluster_kernels: bool = os.environ.get("FT_CLUSTER_KERNELS", "0") == "1"
    strip_kernels: bool = os.environ.get("FT_STRIP_KERNELS", "0") in ("1", "2")      # the 64-plane block's register-stationary form as an option

    def __init__(self, layers: List[int], num_classes: int):
        super().__init__()
        self.layers_cfg = list(layers)
        self.num_classes = num_classes
        self.inplanes = 64
        # trunk (resnet.py:19-27)
        self.conv1 = ConvParams(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = BatchNormParams(64)
        self.relu = ActMarker("relu")
        self.maxpool = ActMarker("maxpool3x3s2")
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self._make_head(num_classes)

    def _make_layer(self, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        mods = [Bottleneck(self.inplanes, planes, stride)]
        self.inplanes = planes * 4
        mods += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*mods)

    # -- the head: what a model adds to the trunk -----------------------------------------------
    def _make_head(self, num_classes: int) -> None:
        raise NotImplementedError

    def _init_head(self) -> None:
        raise NotImplementedError

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        """Record the head's launches behind the trunk (`cur` = layer4's map, `stages` the views behind every stage) and return
        the NCHW fp32 heat maps they write."""
        raise NotImplementedError

    # -- plan construction ----------------------------------------------------------------------
    def _check_input_size(self, H: int, W: int) -> None:
        if H % 32 or W % 32:
            raise FlowtrackHipError(f"input {H}x{W}: height and width must be multiples of 32")

    def _record_net(self, prog, x_static, dtype, device):
        """The ResNet trunk and, through _record_head, the model's head."""
        B, _, H, W = x_static.shape
        cur = new_act(B, H // 4, W // 4, 64, dtype, device)
        # conv1 + bn1 + relu + maxpool (resnet.py:19-23)
        stem = self.record_stem(prog, "conv1", "+maxpool", self.conv1, self.bn1, x_static, cur, dtype, device)
        split = self.split_lanes if (dtype == torch.float16 and B % 2 == 0 and B >= 32 and self._stem_pools(dtype) and not self.full_stage_maps) else 0
        if split == 2:
            stem(0, B // 2)             # (the other half: on the second lane)
        else:
            stem()

        # FT_SPLIT_LANES=1 (dev, measured in profiles/README.md): layer1 + layer2 as TWO half-batch lanes (parallel graph branches).
        # Their fused blocks are phase-locked across the chip — every workgroup reads its input, then multiplies, then writes, at
        # the same time, so HBM idles while the matrix pipe runs and vice versa; two lanes half a block apart overlap them.
        stages = _Stages({"stem": cur})         # activation views behind each stage (diagnostics: tests/error_budget.py)
        trunk = (self.layer1, self.layer2, self.layer3, self.layer4)
        seam = None                    # output view of this stage's entry block when the previous stage's exit form recorded it
        for li, layer in enumerate(trunk, start=1):
            if li > 1 and seam is None:
                stages[f"layer{li - 1}"] = cur
            elif li > 1:
                stages.absent[f"layer{li - 1}"] = ("this plan records the stage's last block in the exit form, which writes only the even pixels of "
                                                   "its output (the full map exists only if the first-call benchmark kept today's launches): for the "
                                                   "map, build the model with fuse_stage_exit = False (FT_FUSE_STAGE_EXIT=0)")
            if split and li == 1:
                # (split == 2: the side lane starts with its half of the stem: half a block of useful delay, the lanes' memory and
                # matrix phases interleave)
                cur = self._record_lanes(prog, [(f"layer{lj}.{bi}", blk) for lj, lay in ((1, self.layer1), (2, self.layer2)) for bi, blk in enumerate(lay)],
                                         cur, (lambda: stem(B // 2, B)) if split == 2 else None)
                continue
            if split and li == 2:
                continue
            if self.split_lanes4 and li == 4 and dtype == torch.float16 and B % 2 == 0 and B >= 32:
                # FT_SPLIT_LANES4=1 (dev): layer4 as two half-batch lanes.  Its nine launches are small (15-30 us each, of which ~6 us
                # are the launch's ramp with the chip mostly idle: cd_phases.py shows 10-us workgroup lifetimes in 16-us kernels); two
                # lanes fill each other's ramps, and halving the pixels halves the workgroups, not the weight bytes per workgroup.
                # MEASURED (two interleaved bench runs): 56.37 / 55.82 -> 53.75 / 53.79 k crops/s: off.
                cur = self._record_lanes(prog, [(f"layer4.{bi}", blk) for bi, blk in enumerate(layer)], cur)
                continue
            for bi, blk in enumerate(layer):
                if bi == 0 and seam is not None:
                    cur, seam = seam, None
                    continue
                name = f"layer{li}.{bi}"
                out = new_act(B, cur.H // blk.stride, cur.W // blk.stride, blk.conv1.cout * 4, dtype, device)
                if bi == len(layer) - 1 and bi > 0 and li < 4 and not split and not self.full_stage_maps:
                    seam = self._record_stage_exit(prog, name, blk, f"layer{li + 1}.0", trunk[li][0], cur, out, dtype, device)
                    if seam is not None:
                        continue
                cur = self._record_trunk_block(prog, name, blk, cur, out)

        stages["layer4"] = cur
        heatmaps = self._record_head(prog, stages, cur, dtype, device)
        return stages, heatmaps

    def _record_lanes(self, prog, blocks, cur: ActView, side_first=None) -> ActView:
        """The chain `blocks` = [(name, blk), ...] from view `cur` as two half-batch lanes (parallel graph branches): the first half
        on the main lane, the second on the side lane, behind `side_first()` where given.  Returns the chain's full-batch output."""
        B, chain = cur.N, []
        hh, ww = cur.H, cur.W
        for name, blk in blocks:
            hh, ww = hh // blk.stride, ww // blk.stride
            chain.append((name, blk, new_act(B, hh, ww, blk.conv1.cout * 4, cur.t.dtype, cur.t.device)))

        def lane(lo, hi):
            c = cur.batch_slice(lo, hi)
            for name, blk, out_full in chain:
                c = self._record_trunk_block(prog, name, blk, c, out_full.batch_slice(lo, hi))
        prog.fork()
        lane(0, B // 2)
        with prog.side():
            if side_first is not None:
                side_first()
            lane(B // 2, B)
        prog.join()
        return chain[-1][2]

    def _record_trunk_block(self, prog, name: str, blk, cur: ActView, out: ActView) -> ActView:
        """One trunk block (stride on its 3x3) in every form this model's switches offer: resnet.record_block."""
        forms = (("fused", "entry", "head", "head2") if self.fuse_bottleneck else ()) + (("shortcut",) if self.fuse_shortcut else ()) + \
            (("cluster",) if self.cluster_kernels else ()) + (("strips",) if self.strip_kernels else ())
        return record_block(self, prog, name, blk, cur, out, stride=blk.stride, stride_on="conv2", forms=forms)

    def _record_stage_exit(self, prog, name: str, blk, nname: str, nblk, cur, out, dtype, device):
        """The seam between two stages: `blk` = the stage's last identity block (from `cur` into `out`), `nblk` = the stride-2 entry
        block of the next stage.  Nothing but nblk.conv1 and nblk's stride-2 shortcut reads `out`, so where ft_bottleneck_exit_fwd
        covers the pair (fp16, 256 -> 64 -> 64 -> 256 then 256 -> 128: layer1 -> layer2) two forms of BOTH blocks are recorded and
        the first-call benchmark keeps one:
          "fused"  blk + nblk.conv1 as one launch that writes t1 and the even pixels of blk's output as a compact half-size map,
                   then nblk.conv2 and the K-concatenated conv3 + shortcut, which reads the compact map at stride 1;
          "convs"  the launches resnet.record_block gives the two blocks (nblk.conv1 a launch of its own).
        Returns nblk's output view, or None when the exit form does not apply (nothing recorded then)."""
        if not (self.fuse_stage_exit and self.fuse_bottleneck and self.fuse_shortcut) or dtype != torch.float16:
            return None
        if len(blk.downsample) or blk.stride != 1 or nblk.stride != 2 or not len(nblk.downsample) or cur.H % 2 or cur.W % 2:
            return None
        B, mk = cur.N, dict(dtype=dtype, device=device)
        nplanes = nblk.conv1.cout
        c1 = self.fused(name + ".conv1", blk.conv1.weight, bn=blk.bn1.as_dict(), act="relu", **mk)
        c2 = self.fused(name + ".conv2", blk.conv2.weight, stride=1, pad=1, bn=blk.bn2.as_dict(), act="relu", **mk)
        c3 = self.fused(name + ".conv3", blk.conv3.weight, bn=blk.bn3.as_dict(), act="relu", **mk)
        n1 = self.fused(nname + ".conv1", nblk.conv1.weight, bn=nblk.bn1.as_dict(), act="relu", **mk)
        n2 = self.fused(nname + ".conv2", nblk.conv2.weight, stride=2, pad=1, bn=nblk.bn2.as_dict(), act="relu", **mk)
        t1 = new_act(B, cur.H, cur.W, nplanes, dtype, device)
        y_even = new_act(B, cur.H // 2, cur.W // 2, cur.C, dtype, device)
        if not bottleneck_exit_fusable(c1, c2, c3, n1, cur, y_even, t1, "even"):
            return None
        t2 = new_act(B, cur.H // 2, cur.W // 2, nplanes, dtype, device)
        nout = new_act(B, cur.H // 2, cur.W // 2, nplanes * 4, dtype, device)
        # the same GEMM as the block recorder's, its shortcut operand read at stride 1 from the compact map
        sc = self.fused_shortcut(nname + ".conv3+downsample", nblk, 1, key_suffix="@even", **mk)

        def exit_form():
            record_bottleneck_exit(prog, c1, c2, c3, n1, cur, y_even, t1, f"{name}.fused+{nname}.conv1", "even")
            n2.record(prog, t1, t2)
            sc.record(prog, t2, y_even, nout)

        def block_form():
            self._record_trunk_block(prog, name, blk, cur, out)
            self._record_trunk_block(prog, nname, nblk, out, nout)
        # a choice of the "bottleneck" family, with that family's option names: "fused" = the block fused with the conv behind it
        # (the exit form), "convs" = that conv stays a launch of its own (today's launches of the two blocks)
        prog.choice(f"bottleneck|exit,{B},{cur.H},{cur.W},{cur.C},{nplanes},{cur.cstride}", {"fused": exit_form, "convs": block_form},
                    only="fused" if self.fuse_stage_exit == "force" else None)
        return nout


class DeconvResnet(PoseResnet):
    """ResNet trunk + 3 x ConvTranspose(4,2,1) + 1x1 heatmap conv (pose_deconv.py:12-63)."""
    supports_exact = True
    #: run the 1x1 heatmap conv as the fused tail of the last deconv (fp16 mode); FT_FUSE_HEATMAP=0 keeps it a launch
    fuse_heatmap: bool = os.environ.get("FT_FUSE_HEATMAP", "1") != "0"

    def _make_head(self, num_classes: int) -> None:
        # head (pose_deconv.py:16-30)
        self.deconv_bias = False
        feats = 256
        self.deconv = nn.Sequential(
            ConvTransposeParams(2048, feats, bias=False), BatchNormParams(feats), ActMarker("relu"),
            ConvTransposeParams(feats, feats, bias=False), BatchNormParams(feats), ActMarker("relu"),
            ConvTransposeParams(feats, feats, bias=False), BatchNormParams(feats), ActMarker("relu"))
        self.heatmap = ConvParams(feats, num_classes, 1, bias=True)

    def _init_head(self) -> None:
        # pose_deconv.py:48-63
        for m in self.deconv:
            if isinstance(m, ConvTransposeParams):
                nn.init.normal_(m.weight, std=0.001)
            elif isinstance(m, BatchNormParams):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.heatmap.weight, std=0.001)
        nn.init.constant_(self.heatmap.bias, 0)

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        # head: 3 x (ConvTranspose 4/2/1 + bn + relu), then the 1x1 heatmap conv (pose_deconv.py:43-45) — fused behind
        # the last deconv as its tail in fp16 mode: the [B, 64, 48, 256] map, the largest tensor of the head, never
        # reaches HBM
        B, mk = cur.N, dict(dtype=dtype, device=device)
        fuse_tail = self.fuse_heatmap and dtype == torch.float16 and self.num_classes <= 32 and self.deconv[6].cout in (64, 128, 256)
        heatmaps = None
        for i in (0, 3, 6):
            tail = dict(tail_weight=self.heatmap.weight, tail_bias=self.heatmap.bias) if (i == 6 and fuse_tail) else {}
            dc = self.fused(f"deconv.{i}" + ("+heatmap" if tail else ""), self.deconv[i].weight, transposed=True, stride=2, pad=1,
                            bias=self.deconv[i].bias, bn=self.deconv[i + 1].as_dict(), act="relu", **tail, **mk)
            if tail:
                heatmaps = torch.empty((B, self.num_classes, cur.H * 2, cur.W * 2), dtype=torch.float32, device=device)
                dc.record(prog, cur, heatmaps)
            else:
                nxt = new_act(B, cur.H * 2, cur.W * 2, dc.cout, dtype, device)
                dc.record(prog, cur, nxt)
                cur = nxt
                stages[f"deconv.{i}"] = cur
        if heatmaps is None:
            hm = self.fused("heatmap", self.heatmap.weight, bias=self.heatmap.bias, act=None, **mk)
            heatmaps = torch.empty((B, self.num_classes, cur.H, cur.W), dtype=torch.float32, device=device)
            hm.record(prog, cur, heatmaps)
        return heatmaps


class FpnResnet(FpnHead, PoseResnet):
    """ResNet trunk + the FPN top-down head (fpn_head.FpnHead; pose_fpn.py:48-104): c2..c5 are the maps behind layer1..layer4."""
    full_stage_maps = True


def _bn_relu_deconv(cin: int, cout: int) -> nn.Sequential:
    """_make_deconv of pose_net.py:9-14: BatchNorm (over the INPUT channels), ReLU, ConvTranspose2d(4,2,1) without bias."""
    return nn.Sequential(BatchNormParams(cin), ActMarker("relu"), ConvTransposeParams(cin, cout, bias=False))


class LateralDeconvResnet(PoseResnet):
    """ResNet trunk + three `BatchNorm -> ReLU -> ConvTranspose2d(4,2,1)` steps, each summed with a 1x1 lateral conv of the trunk
    map at its output's scale, + `BatchNorm -> ReLU -> 1x1` heat maps (pose_net.py:30-91).  With c2..c5 the maps behind layer1..layer4:

        p4 = deconv1(c5) + latlayer2(c4),  p3 = deconv2(p4) + latlayer3(c3),  p2 = deconv3(p3) + latlayer4(c2),  heatmaps = heatmap(p2)

    Nothing reads a sum p_j but the BatchNorm + ReLU in front of the next layer, so with (s, b) the fold of that BatchNorm
    (deconv2.0, deconv3.0, heatmap.0) the plan holds only the activated maps:

        a5 = relu(bn_deconv1.0(c5))                       ft_scale_shift_act_nhwc_fwd (c5 is layer4's activated output: no epilogue to fold into)
        a4 = relu(s (deconv1(a5) + lat2(c4)) + b)         one step, likewise a3 and a2
        heatmaps = heatmap.2(a2) + bias                   1x1 conv to NCHW fp32

    A step is recorded in two forms, the first-call benchmark keeps one (`lateral_step_form` forces one):
      "kconcat"         ONE launch: the lateral conv as one more K-run of each parity phase of the transposed conv (FusedLateralDeconv);
      "lateral+deconv"  two launches: the lateral conv writes l = s lat(c) + b, the transposed conv takes scale s, no shift, l as its
                        residual input and the ReLU — on whatever kernel today's dispatch gives a transposed conv with a residual.
    The heat-map conv stays a launch of its own: the fused tail, x2 and a residual all use the same pointer argument."""
    full_stage_maps = True
    #: None: both forms of a top-down step are recorded and the first-call benchmark keeps one; "kconcat" / "lateral+deconv" records
    #: that form only (dev, tests; FT_LATERAL_STEP in the environment)
    lateral_step_form = os.environ.get("FT_LATERAL_STEP") or None
    STEP_FORMS = ("kconcat", "lateral+deconv")

    def _make_head(self, num_classes: int) -> None:
        feats = 256
        for i, cin in ((2, 1024), (3, 512), (4, 256)):                   # lateral layers (pose_net.py:36-40): there is no latlayer1
            setattr(self, f"latlayer{i}", ConvParams(cin, feats, 1, bias=False))
        for j, cin in ((1, 2048), (2, feats), (3, feats)):               # top-down layers (pose_net.py:42-45)
            setattr(self, f"deconv{j}", _bn_relu_deconv(cin, feats))
        self.heatmap = _bn_relu_conv(feats, num_classes, 1)

    def _init_head(self) -> None:
        # pose_net.py:69-91
        for name, m in self.named_modules():
            if "lat" in name:
                if isinstance(m, ConvParams):
                    nn.init.normal_(m.weight, std=0.001)
            elif "deconv" in name:
                if isinstance(m, ConvTransposeParams):
                    nn.init.normal_(m.weight, std=0.001)
                elif isinstance(m, BatchNormParams):
                    nn.init.constant_(m.weight, 1)
                    nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.heatmap[0].weight, 1)
        nn.init.constant_(self.heatmap[0].bias, 0)
        nn.init.normal_(self.heatmap[2].weight, std=0.001)
        nn.init.constant_(self.heatmap[2].bias, 0)

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        form = self.lateral_step_form
        if form is not None and form not in self.STEP_FORMS:
            raise FlowtrackHipError(f"lateral_step_form {form!r}: None or one of {self.STEP_FORMS}")
        B, mk = cur.N, dict(dtype=dtype, device=device)
        feats = self.latlayer2.cout
        ss = self._cached("deconv1.0.scale_shift", dtype, device, lambda: fold_scale_shift(cur.C, cur.C, None, self.deconv1[0].as_dict(), device))
        a = new_act(B, cur.H, cur.W, cur.C, dtype, device)
        record_scale_shift_act(prog, cur, a, ss[0], ss[1], "relu")
        stages["a5"] = a
        steps = ((1, 2, "layer3", self.deconv2[0]), (2, 3, "layer2", self.deconv3[0]), (3, 4, "layer1", self.heatmap[0]))
        for j, i, stage, bn_mod in steps:
            dc, lat, c = getattr(self, f"deconv{j}")[2], getattr(self, f"latlayer{i}"), stages[stage]
            bn = bn_mod.as_dict()
            name = f"deconv{j}.2+latlayer{i}"
            out = new_act(B, c.H, c.W, feats, dtype, device)
            kc = self._cached(name, dtype, device, lambda: FusedLateralDeconv(dc.weight, lat.weight, bn, act="relu", label=name, **mk))
            # the two-launch form's layers: l = s lat(c) + b (no activation), then relu(s deconv(a) + l)
            lat_conv = self.fused(f"latlayer{i}.bn", lat.weight, bn=bn, act=None, **mk)
            dc_conv = self._cached(f"deconv{j}.2.scaled", dtype, device, lambda: FusedConv(
                dc.weight, transposed=True, stride=2, pad=1, act="relu", label=f"deconv{j}.2+residual", **mk,
                bn=dict(bn, bias=torch.zeros_like(bn["bias"]), running_mean=torch.zeros_like(bn["running_mean"]))))
            lbuf = new_act(B, c.H, c.W, feats, dtype, device)

            def kconcat_form(kc=kc, a=a, c=c, out=out):
                kc.record(prog, a, c, out)

            def two_form(lat_conv=lat_conv, dc_conv=dc_conv, a=a, c=c, out=out, lbuf=lbuf):
                lat_conv.record(prog, c, lbuf)
                dc_conv.record(prog, a, out, residual=lbuf)
            prog.choice(f"lateral_step|{B},{a.H},{a.W},{a.C},{c.C},{feats},{a.cstride},{c.cstride},{dtype}",
                        {"kconcat": kconcat_form, "lateral+deconv": two_form}, only=form)
            a = out
            stages[f"a{5 - j}"] = a
        heatmaps = torch.empty((B, self.num_classes, a.H, a.W), dtype=torch.float32, device=device)
        self.fused("heatmap.2", self.heatmap[2].weight, bias=self.heatmap[2].bias, act=None, **mk).record(prog, a, heatmaps)
        return heatmaps
