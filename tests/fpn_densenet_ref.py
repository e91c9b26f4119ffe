"""References of the FPN pose model on DenseNet trunks (lib/pose/models/densenet.py:19-108, pose_fpn.py:106-151), shared by
tests/test_fpn_densenet_cpu.py, test_preact_conv_gpu.py, test_fpn_densenet_gpu.py and tests/golden/make_fpn_densenet_golden.py.

  fpn_densenet_forward  torch-CPU fp32 functional restatement of FPN_Densenet.forward, one torch.nn.functional call per op of the
                        reference; pinned against the imported reference by make_fpn_densenet_golden.py.
  preact_conv1x1_ref    float64 restatement of ft_preact_conv1x1_fwd's contract (include/flowtrack_hip.h) with the derived bound of
                        one output element's error.
  PREACT_CASES          the case table of the kernel's tests.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from fpn_ref import _bn_relu_conv, _upsample_add
from oracle import pose_ref

#: depth -> (num_init_features, growth_rate, block_config): densenet.py:150-153
DENSENET = {121: (64, 32, (6, 12, 24, 16)), 169: (64, 32, (6, 12, 32, 32)), 201: (64, 32, (6, 12, 48, 32)), 161: (96, 48, (6, 12, 36, 24))}


def planes(depth: int):
    """Channels of c2..c5 (DenseNet.planes, densenet.py:84-94)."""
    c, growth, cfg = DENSENET[depth]
    out = []
    for i, n in enumerate(cfg):
        c += n * growth
        out.append(c)
        if i != len(cfg) - 1:
            c //= 2
    return out


@torch.no_grad()
def fpn_densenet_forward(sd, x, depth=121, return_features=False):
    """sd: state_dict of fpn('densenet<depth>', K) (CPU tensors); x [B,3,H,W] -> heat maps [B,K,H/4,W/4] fp32 (pose_fpn.py:124-151)."""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    _, _, cfg = DENSENET[depth]
    x = F.relu(pose_ref._bn(sd, "norm0", F.conv2d(x.float(), sd["conv0.weight"], stride=2, padding=3)))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    c = []
    for bi, nlayers in enumerate(cfg, start=1):
        for li in range(1, nlayers + 1):
            p = f"denseblock{bi}.denselayer{li}"
            t = F.conv2d(F.relu(pose_ref._bn(sd, p + ".norm1", x)), sd[p + ".conv1.weight"])
            t = F.conv2d(F.relu(pose_ref._bn(sd, p + ".norm2", t)), sd[p + ".conv2.weight"], padding=1)
            x = torch.cat([x, t], 1)
        c.append(x)
        if bi != len(cfg):
            p = f"transition{bi}"
            x = F.avg_pool2d(F.conv2d(F.relu(pose_ref._bn(sd, p + ".norm", x)), sd[p + ".conv.weight"]), kernel_size=2, stride=2)
    c2, c3, c4, c5raw = c
    c5 = F.relu(pose_ref._bn(sd, "norm5", c5raw))
    p5 = F.conv2d(c5, sd["latlayer1.weight"])
    p4 = _bn_relu_conv(sd, "toplayer1", _upsample_add(p5, F.conv2d(c4, sd["latlayer2.weight"])), padding=1)
    p3 = _bn_relu_conv(sd, "toplayer2", _upsample_add(p4, F.conv2d(c3, sd["latlayer3.weight"])), padding=1)
    p2 = _bn_relu_conv(sd, "toplayer3", _upsample_add(p3, F.conv2d(c2, sd["latlayer4.weight"])), padding=1)
    out = _bn_relu_conv(sd, "heatmap", p2)
    # layer1..layer4: the raw block outputs (the sources of c2..c5: c5 itself is relu(norm5(layer4)) and is never stored on the HIP path)
    feats = {"layer1": c2, "layer2": c3, "layer3": c4, "layer4": c5raw, "p5": p5, "p4": p4, "p3": p3, "p2": p2}
    return (out, feats) if return_features else out


# ---- the kernel's contract -------------------------------------------------------------------------------------------------------
def preact_conv1x1_ref(x, w, pre_scale, pre_shift, post_scale=None, post_shift=None, pool=False, relu=False, fp16=False):
    """x [N,H,W,Cin] (the values the kernel reads, any float dtype: they enter exactly), w [Cout,Cin] (fp32 / float64 master
    weights; the fp16 mode rounds them once when it packs), pre_* [Cin], post_* [Cout] or None -> (want, bound), float64
    [N,Ho,Wo,Cout].  want is the contract evaluated in float64 with NO rounding anywhere; bound is the largest |result - want| of
    any evaluation that follows the contract, with u = 2^-24 (fp32) and h = 2^-11 (fp16), per output element:

      a_c, the operand: one fp32 fma (relative u of its result; the ReLU and the exact 0.25 add nothing), pooled: three more fp32
          adds of non-negative terms (relative u each), fp16: one rounding to fp16 (relative h, or 2^-25 absolute in the
          subnormal range)                                              -> |da_c| <= a_c ((1 + u)^(1 + 3 pool) (1 + h) - 1) + 2^-25 [fp16]
      w_c: fp16 rounds it once                                          -> |dw_c| <= h |w_c| + 2^-25 [fp16]
      the sum of K products in fp32, in any order (an MFMA's included): every partial sum is at most S' = sum |a'_c w'_c| of the
          rounded operands, one rounding of u per add (the fp16 products are exact in fp32; an fp32 fma rounds once per term)
                                                                        -> K u S'
      epilogue: the fma with post_scale / post_shift (relative u of its result), the rounding to the output type
    """
    x = x.detach().cpu().double()
    w = w.detach().cpu().double()
    ps, pb = pre_scale.detach().cpu().double(), pre_shift.detach().cpu().double()
    u, h = 2.0 ** -24, 2.0 ** -11
    r = torch.relu(x * ps + pb)
    if pool:
        N, H, W, C = r.shape
        r = r[:, :H // 2 * 2, :W // 2 * 2]
        r = 0.25 * ((r[:, 0::2, 0::2] + r[:, 0::2, 1::2]) + (r[:, 1::2, 0::2] + r[:, 1::2, 1::2]))
    K = w.shape[1]
    rel_a = (1.0 + u) ** (4 if pool else 1) * ((1.0 + h) if fp16 else 1.0) - 1.0
    da = r * rel_a + (2.0 ** -25 if fp16 else 0.0)
    dw = (w.abs() * h + 2.0 ** -25) if fp16 else torch.zeros_like(w)
    acc = r @ w.t()
    S = r @ w.abs().t()
    # |a' w' - a w| <= |da| |w| + (|a| + |da|) |dw|;  S' <= S + that
    d_ops = da @ w.abs().t() + (r + da) @ dw.t()
    d_acc = d_ops + K * u * (S + d_ops)
    if post_scale is not None:
        qs, qb = post_scale.detach().cpu().double(), post_shift.detach().cpu().double()
        want = acc * qs + qb
        d = d_acc * qs.abs() + u * (want.abs() + d_acc * qs.abs())
    else:
        want, d = acc, d_acc
    if relu:
        want = torch.relu(want)         # (1-Lipschitz: the bound carries over)
    d = d + (h * (want.abs() + d) + 2.0 ** -25 if fp16 else u * (want.abs() + d))
    return want, d


# (name, N, H, W, Cin, x_cstride, Cout, y_cstride, y_coff, pool): the rows of the kernel's tests (tests/test_preact_conv_gpu.py)
PREACT_CASES = (
    ("a_one_pixel", 1, 1, 1, 32, 32, 32, 32, 0, False),            # one K step (fp16: half a chunk), one pixel
    ("b_masked_tail", 1, 5, 7, 160, 256, 128, 192, 32, False),     # 2.5 chunks, channels [160, 256) NaN, 35 pixels, an output window
    ("c_long_k", 2, 2, 3, 1056, 1056, 128, 128, 0, False),         # 16.5 chunks, 12 pixels: the late-block shape (1-wave workgroups)
    ("d_pool_odd", 1, 5, 7, 64, 64, 32, 32, 0, True),              # 5x7 -> 2x3: the odd row and column take no part
    ("e_pool_k", 2, 4, 4, 256, 256, 128, 128, 0, True),            # pooled, four chunks
    ("f_big_tile", 2, 128, 128, 96, 128, 128, 128, 0, False),      # 32768 pixels: the 4-wave 128-pixel x 128-output workgroups (fp16)
    ("g_big_pool", 2, 258, 254, 64, 64, 128, 160, 32, True),       # 2 x 129 x 127 = 32766 pooled pixels: that shape with the pool, a ragged last tile
)
