"""References of the FPN pose head (lib/pose/models/pose_fpn.py:9-26,48-87), shared by tests/test_fpn_cpu.py, test_fpn_upsample_gpu.py,
test_fpn_gpu.py and tests/golden/make_fpn_golden.py.

  fpn_forward       torch-CPU fp32 functional restatement of FPN_Resnet.forward, one torch.nn.functional call per op of the reference
                    (trunk blocks from oracle/pose_ref.py); pinned against the imported reference by make_fpn_golden.py.
  upsample_ac_ref   float64 reference of ft_upsample_bilinear_ac_fwd (include/flowtrack_hip.h): the source coordinates and the four
                    weights follow torch's fp32 rule, everything behind them is float64.
  upsample_ac_bound the derived bound of one output element's error against that reference.
  UPSAMPLE_CASES    the case table of the kernel's tests.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pose_ref


def _bn_relu_conv(sd, p, x, padding=0):
    """_make_conv (pose_fpn.py:41-46): BatchNorm (eval) -> ReLU -> conv."""
    return F.conv2d(F.relu(pose_ref._bn(sd, p + ".0", x)), sd[p + ".2.weight"], sd.get(p + ".2.bias"), padding=padding)


def _upsample_add(x, y):
    return F.interpolate(x, size=y.shape[2:], mode="bilinear", align_corners=True) + y     # pose_fpn.py:25-26 (F.upsample = F.interpolate)


@torch.no_grad()
def fpn_forward(sd, x, depth=50, return_features=False):
    """sd: state_dict of fpn('resnet<depth>', K) (CPU tensors); x [B,3,H,W] -> heat maps [B,K,H/4,W/4] fp32 (pose_fpn.py:67-87)."""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    x = x.float()
    x = F.relu(pose_ref._bn(sd, "bn1", F.conv2d(x, sd["conv1.weight"], stride=2, padding=3)))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    c = []
    for li, nblocks in enumerate(pose_ref.RESNET_LAYERS[depth], start=1):
        for bi in range(nblocks):
            x = pose_ref._bottleneck(sd, f"layer{li}.{bi}", x, 2 if (bi == 0 and li > 1) else 1)
        c.append(x)
    c2, c3, c4, c5 = c
    p5 = F.conv2d(c5, sd["latlayer1.weight"])
    p4 = _bn_relu_conv(sd, "toplayer1", _upsample_add(p5, F.conv2d(c4, sd["latlayer2.weight"])), padding=1)
    p3 = _bn_relu_conv(sd, "toplayer2", _upsample_add(p4, F.conv2d(c3, sd["latlayer3.weight"])), padding=1)
    p2 = _bn_relu_conv(sd, "toplayer3", _upsample_add(p3, F.conv2d(c2, sd["latlayer4.weight"])), padding=1)
    out = _bn_relu_conv(sd, "heatmap", p2)
    feats = {"layer1": c2, "layer2": c3, "layer3": c4, "layer4": c5, "p5": p5, "p4": p4, "p3": p3, "p2": p2}
    return (out, feats) if return_features else out


# ---- the resize alone ------------------------------------------------------------------------------------------------------------
def ac_axis(n_in: int, n_out: int):
    """Index pair and weights of every output index along one axis, torch's rule for float inputs, each step in fp32:
    r = (n_in - 1) / (n_out - 1) (0 for n_out = 1), src = r * o, i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1."""
    f32 = np.float32
    r = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = (r * np.arange(n_out, dtype=f32)).astype(f32)
    i0 = src.astype(np.int64)
    assert (i0 <= n_in - 1).all()
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def upsample_ac_ref(x: torch.Tensor, ho: int, wo: int, scale=None):
    """x [N,C,hi,wi] (any float dtype; its values enter exactly) -> (want, mag), both float64 [N,C,ho,wo]:
    want = scale[c] * (l0h (l0w a + l1w b) + l1h (l0w c + l1w d)),  mag = the same sum over the magnitudes |a| .. |d| (no scale) —
    the quantity upsample_ac_bound scales the rounding error with."""
    x = x.detach().cpu().double().numpy()
    y0, y1, l0h, l1h = ac_axis(x.shape[2], ho)
    x0, x1, l0w, l1w = ac_axis(x.shape[3], wo)

    def lerp(v):
        top = l0w * v[:, :, y0][:, :, :, x0] + l1w * v[:, :, y0][:, :, :, x1]
        bot = l0w * v[:, :, y1][:, :, :, x0] + l1w * v[:, :, y1][:, :, :, x1]
        return l0h[:, None] * top + l1h[:, None] * bot
    want, mag = lerp(x), lerp(np.abs(x))
    if scale is not None:
        want = want * scale.detach().cpu().double().numpy()[None, :, None, None]
    return torch.from_numpy(want), torch.from_numpy(mag)


def upsample_ac_bound(want: torch.Tensor, mag: torch.Tensor, scale=None, fp16: bool = False) -> torch.Tensor:
    """Largest |result - want| of one output element for ANY fp32 evaluation of the rule in which a term passes through at most
    five roundings.  The weights are the reference's own fp32 numbers, and fp16 / fp32 inputs convert to fp32 exactly, so the
    only errors are those of the arithmetic behind them.  Written out as in the header, each of the four terms l?h * l?w * v
    passes through: its product with the column weight, the add of the column pair, the product with the row weight, the add of
    the row pair, and (with `scale`) the product with scale[c] — five roundings of at most u = 2^-24 relative each (fewer when a
    product and its add are one fused multiply-add, or when a weight is 0 or 1).  The error of a term t is then at most
    ((1 + u)^5 - 1) |t|, and summed over the four terms ((1 + u)^5 - 1) * |scale[c]| * mag with mag = sum of |l?h l?w v|.
    Normal-range values are assumed (products of N(0,1)-sized data and weights that are 0 or at least 2^-24).
    fp16 output adds the one rounding on store: half an fp16 ulp of the computed result, at most 2^-11 (|want| + the fp32 error),
    and 2^-25 absolute in the subnormal range."""
    u = 2.0 ** -24
    b = ((1.0 + u) ** 5 - 1.0) * mag
    if scale is not None:
        b = b * scale.detach().cpu().double().abs().view(1, -1, 1, 1)
    if fp16:
        b = b + 2.0 ** -11 * (want.abs() + b) + 2.0 ** -25
    return b


# (name, N, C, hi, wi, ho, wo): the rows of the kernel's tests
UPSAMPLE_CASES = (
    ("exact2x_fpn", 1, 8, 3, 2, 6, 4),
    ("c256_n3", 3, 256, 4, 3, 8, 6),
    ("half_weights", 2, 24, 5, 4, 9, 7),          # out = 2 in - 1: every weight is 0, 0.5 or 1
    ("ratio0", 1, 16, 1, 1, 2, 2),
    ("identity", 3, 40, 4, 4, 4, 4),
    ("to_1x1", 2, 8, 3, 5, 1, 1),
    ("non_integer", 1, 32, 2, 2, 7, 5),
    ("odd_c_tail", 2, 13, 3, 4, 5, 9),            # C no multiple of the 16-byte group: the element-wise last group
    ("multi_block", 1, 64, 9, 7, 33, 21),         # 33 x 21 pixels x 8 (fp16) / 16 (fp32) groups: 22 / 44 workgroups of 256 threads
)
