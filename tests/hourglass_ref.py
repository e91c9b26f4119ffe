"""References of the stacked-hourglass pose model (lib/pose/models/hourglass.py) and of its two seam kernels, shared by
tests/test_hourglass_cpu.py, test_hourglass_ops_gpu.py, test_hourglass_gpu.py and tests/golden/make_hg_golden.py.

  hg_forward      torch-CPU fp32 functional restatement of HourglassNet.forward, one torch.nn.functional call per op of the
                  reference; pinned against the imported reference by make_hg_golden.py (1e-5 of each map's range).
  stack_tol       the per-stack heat-map tolerance of the fp32 tests: max(1e-3, 1.2e-4 * range) — the project's fp32 bar (1e-3 on the
                  FPN fixture's range of 9.0) carried over to the hourglass's larger ranges.
  down_ref        float64 / exact numpy reference of ft_hourglass_down_fwd (include/flowtrack_hip.h).
  up_ref          float64 reference of ft_hourglass_up_fwd's sum: the resize of fpn_ref.upsample_ac_ref plus the skip map.
  up_bound        the derived bound of one sum element's error against up_ref.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import fpn_ref

DEPTH = 4


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _conv(sd, p, x, padding=0, stride=1):
    return F.conv2d(x, sd[p + ".weight"], sd.get(p + ".bias"), stride=stride, padding=padding)


class _Peak:
    """Largest |activation| seen by a forward (every tensor a module of the reference would output)."""

    def __init__(self):
        self.value = 0.0

    def __call__(self, t):
        self.value = max(self.value, float(t.abs().max()))
        return t


def _block(sd, p, x, see):
    """bottleneck.forward (hourglass.py:33-45): 'preact' where the block has one, 'no_preact' otherwise."""
    a = F.relu(see(_bn(sd, p + ".preact.0", x))) if (p + ".preact.0.weight") in sd else x
    t = F.relu(see(_bn(sd, p + ".branch.1", see(_conv(sd, p + ".branch.0", a)))))
    t = F.relu(see(_bn(sd, p + ".branch.4", see(_conv(sd, p + ".branch.3", t, padding=1)))))
    t = see(_conv(sd, p + ".branch.6", t))
    y = see(_conv(sd, p + ".shortcut", x)) if (p + ".shortcut.weight") in sd else x
    return see(t + y)


def _chain(sd, p, x, see):
    k = 0
    while f"{p}.{k}.branch.0.weight" in sd:
        x = _block(sd, f"{p}.{k}", x, see)
        k += 1
    assert k > 0, p
    return x


def _level(sd, p, n, x, see):
    """Hourglass._hourglass_forward (hourglass.py:110-121)."""
    q = f"{p}.{n - 1}"
    up1 = _chain(sd, q + ".0", x, see)
    low1 = _chain(sd, q + ".1", F.max_pool2d(x, kernel_size=2, stride=2), see)
    low2 = _level(sd, p, n - 1, low1, see) if n > 1 else _chain(sd, q + ".3", low1, see)
    low3 = _chain(sd, q + ".2", low2, see)
    return see(F.interpolate(low3, size=up1.shape[2:], mode="bilinear", align_corners=True) + up1)


@torch.no_grad()
def hg_forward(sd, x, num_stacks, return_peak=False):
    """sd: state_dict of hg(K, num_stacks) (CPU tensors); x [B,3,H,W] -> list of num_stacks heat maps [B,K,H/4,W/4] fp32
    (hourglass.py:203-225); return_peak: also the largest |activation|."""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    see = _Peak()
    x = F.relu(see(_bn(sd, "pre.1", see(_conv(sd, "pre.0", x.float(), padding=3, stride=2)))))
    x = _chain(sd, "res1", x, see)
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = _chain(sd, "res3", _chain(sd, "res2", x, see), see)
    out = []
    for i in range(num_stacks):
        y = _level(sd, f"hg.{i}.hg", DEPTH, x, see)
        y = _chain(sd, f"res.{i}", y, see)
        y = F.relu(see(_bn(sd, f"proj.{i}.1", see(_conv(sd, f"proj.{i}.0", y)))))
        hm = see(_conv(sd, f"heatmap.{i}", y))
        out.append(hm)
        if i < num_stacks - 1:
            x = see(x + see(_conv(sd, f"proj_.{i}", y)) + see(_conv(sd, f"heatmap_.{i}", hm)))
    return (out, see.value) if return_peak else out


def stack_tol(rng: float) -> float:
    return max(1e-3, 1.2e-4 * float(rng))


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
def affine_relu_exact(x: np.ndarray, scale: np.ndarray, shift: np.ndarray, dtype) -> np.ndarray:
    """dtype(relu(scale[c] * x + shift[c])) in float64, channels last: the kernel's value wherever the fp32 fma is exact (the
    integer-grid cases: small integers times powers of two plus multiples of 0.5)."""
    return np.maximum(x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64), 0.0).astype(dtype)


def down_ref(x: np.ndarray):
    """x [N,H,W,C] -> pool [N,H//2,W//2,C] of x's dtype, every value one of the window's four (nn.MaxPool2d(2, stride=2): an odd
    last row or column takes no part)."""
    N, H, W, C = x.shape
    v = x[:, :H // 2 * 2, :W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C)
    return v.max(axis=(2, 4))


def up_ref(skip: torch.Tensor, low: torch.Tensor):
    """skip [N,H,W,C], low [N,hl,wl,C] (any float dtype; values enter exactly) -> (want, mag) float64 [N,H,W,C]: want = skip +
    bilerp_ac(low), mag = the resize's sum of magnitudes (fpn_ref.upsample_ac_ref)."""
    bil, mag = fpn_ref.upsample_ac_ref(low.permute(0, 3, 1, 2), skip.shape[1], skip.shape[2])
    return skip.detach().cpu().double() + bil.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def up_bound(want: torch.Tensor, mag: torch.Tensor, fp16: bool) -> torch.Tensor:
    """Largest |sum - want| of one element: the resize's fp32 error (fpn_ref.upsample_ac_bound without a scale: ((1 + u)^5 - 1) mag,
    u = 2^-24), one more fp32 rounding for the add of the skip value, and for fp16 the rounding on store (half an fp16 ulp of the
    computed sum, 2^-25 absolute in the subnormal range)."""
    u = 2.0 ** -24
    b = ((1.0 + u) ** 5 - 1.0) * mag
    b = b + u * (want.abs() + b)
    if fp16:
        b = b + 2.0 ** -11 * (want.abs() + b) + 2.0 ** -25
    return b
