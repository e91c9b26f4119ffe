"""The FPN pose model on a DenseNet-BC trunk (pose_fpn.py:106-151, densenet.py:57-108): FpnDensenet and its parameter layout."""
from __future__ import annotations

import os
import re

import torch.nn as nn

from ..hip_ops import ActView, FlowtrackHipError, PreactConv1x1, new_act
from ..params import ActMarker, BatchNormParams, ConvParams
from .fpn_head import FpnHead
from .host import PoseHost, PooledStem, _Stages

#: depth -> (num_init_features, growth_rate, block_config) (densenet.py:150-153)
densenet_dict = {121: (64, 32, [6, 12, 24, 16]), 169: (64, 32, [6, 12, 32, 32]), 201: (64, 32, [6, 12, 48, 32]), 161: (96, 48, [6, 12, 36, 24])}


class DenseLayer(nn.Module):
    """Parameter layout of _DenseLayer (densenet.py:19-30): norm1 -> relu1 -> conv1 (1x1 to bn_size * growth) -> norm2 -> relu2 -> conv2
    (3x3 to growth); its output is concatenated behind its input."""

    def __init__(self, cin: int, growth: int, bn_size: int):
        super().__init__()
        self.norm1, self.relu1 = BatchNormParams(cin), ActMarker("relu")
        self.conv1 = ConvParams(cin, bn_size * growth, 1, bias=False)
        self.norm2, self.relu2 = BatchNormParams(bn_size * growth), ActMarker("relu")
        self.conv2 = ConvParams(bn_size * growth, growth, 3, padding=1, bias=False)


class DenseBlock(nn.Module):
    """_DenseBlock (densenet.py:39-44): denselayer1 .. denselayerN, layer i on cin + (i - 1) growth channels."""

    def __init__(self, num_layers: int, cin: int, growth: int, bn_size: int):
        super().__init__()
        for i in range(num_layers):
            self.add_module(f"denselayer{i + 1}", DenseLayer(cin + i * growth, growth, bn_size))

    def layers(self):
        return list(self.children())


class Transition(nn.Module):
    """_Transition (densenet.py:47-54): norm -> relu -> conv (1x1, halves the channels) -> AvgPool2d(2, 2)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.norm, self.relu = BatchNormParams(cin), ActMarker("relu")
        self.conv = ConvParams(cin, cout, 1, bias=False)
        self.pool = ActMarker("avgpool2x2s2")


class FpnDensenet(FpnHead, PooledStem, PoseHost):
    """DenseNet-BC trunk + the FPN head (fpn_head.FpnHead): c2..c5 are the four dense blocks' buffers.

    A dense block is ONE NHWC buffer [B, H, W, inplanes + L * growth]: every layer reads the channel window [0, cin) and writes its
    `growth` new channels into the window behind it, so the reference's torch.cat never runs.  A dense layer is two launches:
        t = relu(norm2(conv1(relu(norm1(block[:cin])))))      ft_preact_conv1x1_fwd: norm1 + ReLU on the GEMM's input operand (norm1
                                                               belongs to the layer that reads the concat: no producer can fold it)
        block[cin : cin + growth] = conv2(t)                   the 3x3 conv of today's path
    The first is recorded in two forms, the first-call benchmark keeps one per shape (`dense_layer_form` pins one):
      "preact"        the one launch above;
      "affine+igemm"  ft_scale_shift_act_nhwc_fwd writes relu(norm1(block[:cin])), ft_conv2d_fwd reads it.
    A transition is one ft_preact_conv1x1_fwd launch with pool = 1 (the 2x2 average commutes with the 1x1 conv, so it runs on the
    GEMM's input and the GEMM has a quarter of the pixels) into channels [0, inplanes / 2) of the next block's buffer; p5 =
    latlayer1(relu(norm5(block4))) is one more, so c5 is never written.  latlayer2..4 read the raw block buffers c4, c3, c2."""
    #: None: both forms of a dense layer's first launch are recorded and the first-call benchmark keeps one per shape; "preact" /
    #: "affine+igemm" records that form only (dev, tests; FT_DENSE_LAYER in the environment)
    dense_layer_form = os.environ.get("FT_DENSE_LAYER") or None
    LAYER_FORMS = ("preact", "affine+igemm")
    bn_size = 4
    kaiming_args = {}       # densenet.py:141-148: kaiming_normal_ as it is (fan_in)

    def __init__(self, num_init_features: int, growth_rate: int, block_config, num_classes: int):
        super().__init__()
        self.num_classes, self.growth_rate, self.block_config = num_classes, growth_rate, list(block_config)
        self.conv0 = ConvParams(3, num_init_features, 7, stride=2, padding=3, bias=False)
        self.norm0 = BatchNormParams(num_init_features)
        self.relu0 = ActMarker("relu")
        self.pool0 = ActMarker("maxpool3x3s2")
        self.inplanes, self.planes = num_init_features, []
        for i, n in enumerate(self.block_config):
            setattr(self, f"denseblock{i + 1}", DenseBlock(n, self.inplanes, growth_rate, self.bn_size))
            self.inplanes += n * growth_rate
            self.planes.append(self.inplanes)
            if i != len(self.block_config) - 1:
                setattr(self, f"transition{i + 1}", Transition(self.inplanes, self.inplanes // 2))
                self.inplanes //= 2
        self.norm5 = BatchNormParams(self.inplanes)
        self._make_head(num_classes, self.planes[::-1])                 # (pose_fpn.py:113-116: latlayer1 reads c5)

    # -- initialisation / loading (densenet.py:122-148) -------------------------------------------
    _OLD_KEY = re.compile(r"^(.*denselayer\d+\.(?:norm|relu|conv))\.((?:[12])\.(?:weight|bias|running_mean|running_var))$")

    @classmethod
    def rewrite_checkpoint_keys(cls, state_dict: dict) -> dict:
        """torchvision's DenseNet checkpoints under this model's names: `features.` stripped, `norm.1` -> `norm1` and likewise
        (densenet.py:126-139)."""
        out = {}
        for key, v in state_dict.items():
            new_key = re.sub(r"^features\.", "", key)
            m = cls._OLD_KEY.match(new_key)
            if m:
                new_key = m.group(1) + m.group(2)
            out[new_key] = v
        return out

    def _check_input_size(self, H: int, W: int) -> None:
        if H % 32 or W % 32 or H < 64 or W < 64:
            raise FlowtrackHipError(f"input {H}x{W}: height and width must be multiples of 32 and at least 64")

    # -- the launch list ----------------------------------------------------------------------------
    def _preact(self, label: str, weight, pre_bn, post_bn, act, dtype, device) -> PreactConv1x1:
        return self._cached(label, dtype, device, lambda: PreactConv1x1(
            weight, pre_bn.as_dict(), post_bn=post_bn.as_dict() if post_bn is not None else None, act=act, dtype=dtype, device=device, label=label))

    def _record_p5(self, prog, cur: ActView, p: ActView, dtype, device) -> None:
        """p5 = latlayer1(relu(norm5(block4))): norm5 + ReLU on the input operand, the activated map c5 is never written."""
        self._preact("norm5+latlayer1", self.latlayer1.weight, self.norm5, None, None, dtype, device).record(prog, cur, p)

    def _record_net(self, prog, x_static, dtype, device):
        form = self.dense_layer_form
        if form is not None and form not in self.LAYER_FORMS:
            raise FlowtrackHipError(f"dense_layer_form {form!r}: None or one of {self.LAYER_FORMS}")
        B, _, H, W = x_static.shape
        mk = dict(dtype=dtype, device=device)
        growth, c0 = self.growth_rate, self.conv0.cout
        h, w = H // 4, W // 4
        buf = new_act(B, h, w, self.planes[0], dtype, device)
        stem_out = ActView(buf.t, c0, 0)
        # conv0 + norm0 + relu0 + pool0 into channels [0, c0) of block 1's buffer
        self.record_stem(prog, "conv0", "+pool0", self.conv0, self.norm0, x_static, stem_out, dtype, device, copy_label="pool0.copy")()
        stages = _Stages({"stem": stem_out})
        cin = c0
        for bi, nlayers in enumerate(self.block_config, start=1):
            block = getattr(self, f"denseblock{bi}")
            t = new_act(B, h, w, self.bn_size * growth, dtype, device)             # conv1's output: read by the next launch only
            scratch = new_act(B, h, w, self.planes[bi - 1], dtype, device) if form != "preact" else None
            for li, layer in enumerate(block.layers(), start=1):
                name = f"denseblock{bi}.denselayer{li}"
                pc = self._preact(name + ".norm1+conv1+norm2", layer.conv1.weight, layer.norm1, layer.norm2, "relu", dtype, device)
                c2 = self.fused(name + ".conv2", layer.conv2.weight, pad=1, act=None, **mk)
                xin = ActView(buf.t, cin, 0)
                prog.choice(f"dense_layer|{B},{h},{w},{cin},{t.C},{buf.cstride},{dtype}",
                            {"preact": lambda: pc.record(prog, xin, t),
                             "affine+igemm": lambda: pc.record_unfused(prog, xin, t, ActView(scratch.t, xin.C, 0))}, only=form)
                c2.record(prog, t, ActView(buf.t, growth, cin))
                cin += growth
            stages[f"layer{bi}"] = buf
            if bi != len(self.block_config):
                tr = getattr(self, f"transition{bi}")
                h, w = h // 2, w // 2
                nxt = new_act(B, h, w, self.planes[bi], dtype, device)
                self._preact(f"transition{bi}", tr.conv.weight, tr.norm, None, None, dtype, device).record(prog, buf, ActView(nxt.t, cin // 2, 0), pool=True)
                buf, cin = nxt, cin // 2
        heatmaps = self._record_head(prog, stages, buf, dtype, device)
        return stages, heatmaps
