"""Shared by test_flowops_pinned_cpu.py / _gpu.py: the fixture the reference's own kernels wrote
(tests/golden/flowops_golden.npz, made by tests/golden/make_flowops_golden.py) and the rounding bounds it is compared within.

Bound, per element:  (terms + extra) * 2^-24 * sum |term|.  A sum of n fp32 terms in ANY order is off by at most
(n - 1) u sum|t| (u = 2^-24), the rounding that formed each term adds u sum|t|, together n u sum|t|; `extra` counts the op's
further roundings of the result (a division, a square root, the extra roundings inside each term, the fp32 rounding of the value
compared against) plus one for the second-order terms (n^2 u^2 <= u while n <= 4096).  It is detect_ref.sum_bound at u instead
of 2 u.  Two fp32 computations that each obey the bound differ by at most twice it (GPU kernel vs fixture)."""
import os

import numpy as np

import detect_ref
import flow_grad_ref as ref
from conftest import GOLDEN

G = np.load(os.path.join(GOLDEN, "flowops_golden.npz"))
N_CORR = len([k for k in G.files if k.startswith("corr") and k.endswith(".params")])
N_RS = len([k for k in G.files if k.startswith("rs") and k.endswith(".img")])
N_CN = len([k for k in G.files if k.startswith("cn") and k.endswith(".x")])
CORR_EXACT = (5, 6)            # integer data
RS_EXACT = 2                   # flows in quarters, integer image and gradient
CN_INF = 2                     # holds the all-zero pixel (0, :, 1, 2) and the overflowing one (0, :, 2, 3)


def bound(terms, extra, mag):
    return 0.5 * detect_ref.sum_bound(terms, mag, extra - 1)


def corr(i):
    p = tuple(int(v) for v in G[f"corr{i}.params"])
    return {k: G[f"corr{i}.{k}"] for k in ("in1", "in2", "out", "gout", "gin1", "gin2")}, p


def rs(i):
    return {k: G[f"rs{i}.{k}"] for k in ("img", "flow", "out", "gout", "gimg", "gflow")}


def cn(i):
    return {k: G[f"cn{i}.{k}"] for k in ("x", "out", "gout", "gx")}


def worst(err, bnd):
    """max err / bound; an error where the bound is 0 counts as infinite."""
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(r.max()) if r.size else 0.0


# ---- correlation -----------------------------------------------------------------------------------------------------------
def corr_fwd_bound(c, p):
    """terms k*k*C products; extra: the division by nelems, the compared value's own rounding, second order."""
    from oracle import ops_ref
    pad, k, md, s1, s2 = p
    mag = ops_ref.correlation_np(np.abs(c["in1"]), np.abs(c["in2"]), *p).astype(np.float64)
    return bound(k * k * c["in1"].shape[1], 3, mag)


_BWD = {}


def corr_bwd_loops(i):
    """(gi1, gi2, bound1, bound2) of the float64 restatement of the reference's backward loops, computed once per case.
    terms: output channels * the window of output pixels (at most k*k / stride1^2, k*k taken); extra as in the forward."""
    if i not in _BWD:
        c, p = corr(i)
        g1, g2 = ref.correlation_bwd_loops(c["in1"], c["in2"], c["gout"], *p)
        m1, m2 = ref.correlation_bwd_loops(np.abs(c["in1"]), np.abs(c["in2"]), np.abs(c["gout"]), *p)
        n = c["gout"].shape[1] * p[1] * p[1]
        _BWD[i] = (g1, g2, bound(n, 3, m1), bound(n, 3, m2))
    return _BWD[i]


def corr_lattice(shape, s1):
    """[B, C, H, W] mask of the input pixels the backward kernels' blocks are meant to write: multiples of stride1."""
    on = np.zeros(shape, dtype=bool)
    on[:, :, ::s1, ::s1] = True
    return on


def corr_stray_targets(shape, s1):
    """Elements that the flat index c*H*W + (yi*s1)*W + xi*s1 of a block with yi*s1 >= H or xi*s1 >= W lands on (the blocks
    form an [H, W, C] grid whatever the stride); indices past the tensor are dropped."""
    B, C, H, W = shape
    hit = np.zeros(shape, dtype=bool).reshape(B, -1)
    for c in range(C):
        for yi in range(H):
            for xi in range(W):
                f = c * H * W + yi * s1 * W + xi * s1
                if (yi * s1 >= H or xi * s1 >= W) and f < C * H * W:
                    hit[:, f] = True
    return hit.reshape(shape)


def corr_is_adjoint_case(p):
    """The reference's backward is the gradient of its forward for kernel_size 1 and stride1 1 only: at k = 3 gradInput1 sums the
    wrong output window, and for stride1 > 1 both kernels visit input pixels at multiples of stride1 alone."""
    return p[1] == 1 and p[3] == 1


def corr_adjoint(i):
    import torch
    c, p = corr(i)
    a = torch.from_numpy(c["in1"]).double().requires_grad_()
    b = torch.from_numpy(c["in2"]).double().requires_grad_()
    ref.correlation_fwd(a, b, *p).backward(torch.from_numpy(c["gout"]).double())
    return a.grad.numpy(), b.grad.numpy()


# ---- resample2d ------------------------------------------------------------------------------------------------------------
def rs_geometry(flow, H, W):
    """fp32 coordinates as the kernels form them, and the clamped neighbour indices."""
    flow = np.asarray(flow, dtype=np.float32)
    xf = (np.arange(W, dtype=np.float32)[None, None, :] + flow[:, 0]).astype(np.float64)
    yf = (np.arange(H, dtype=np.float32)[None, :, None] + flow[:, 1]).astype(np.float64)
    fx, fy = np.floor(xf), np.floor(yf)
    idx = dict(xL=np.clip(fx, 0, W - 1).astype(np.int64), xR=np.clip(fx + 1, 0, W - 1).astype(np.int64),
               yT=np.clip(fy, 0, H - 1).astype(np.int64), yB=np.clip(fy + 1, 0, H - 1).astype(np.int64))
    return xf, yf, fx, fy, idx


def _taps(img, idx):
    B, C = img.shape[:2]
    bi, ci = np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None]
    t = lambda yy, xx: img[bi, ci, yy[:, None], xx[:, None]]  # noqa: E731
    return t(idx["yT"], idx["xL"]), t(idx["yT"], idx["xR"]), t(idx["yB"], idx["xL"]), t(idx["yB"], idx["xR"])


def rs_fwd_bound(r):
    """4 terms (double weights times the tap, each addition rounded to fp32); extra: compared value's rounding, second order."""
    img = np.abs(r["img"]).astype(np.float64)
    B, C, H, W = img.shape
    xf, yf, fx, fy, idx = rs_geometry(r["flow"], H, W)
    a, b = (xf - fx)[:, None], (yf - fy)[:, None]
    TL, TR, BL, BR = _taps(img, idx)
    return bound(4, 2, (1 - a) * (1 - b) * TL + a * (1 - b) * TR + (1 - a) * b * BL + a * b * BR)


def rs_negative_sources(r):
    """[B, H, W]: source pixels where the reference's backward weights (alpha = xf - int(xf)) differ from its forward's
    (xf - floor(xf)): a negative, non-integer coordinate."""
    _, _, H, W = r["img"].shape
    xf, yf, fx, fy, _ = rs_geometry(r["flow"], H, W)
    return ((xf < 0) & (xf != fx)) | ((yf < 0) & (yf != fy))


def rs_bwd_bounds(r):
    """(bound of gimg, bound of gflow, mask of gimg elements that a negative-coordinate source pixel scatters into).
    gimg: n_i atomic terms land on element i, each (1 - alpha), (1 - beta), their product and the product with g rounded:
    terms n_i, extra 4 + 2.  gflow: 4 C terms, each gamma, 1 - gamma and two products rounded: extra 4 + 2."""
    img, g = np.abs(r["img"]).astype(np.float64), np.abs(r["gout"]).astype(np.float64)
    B, C, H, W = img.shape
    xf, yf, fx, fy, idx = rs_geometry(r["flow"], H, W)
    al, be = xf - np.trunc(xf), yf - np.trunc(yf)                             # in (-1, 1): the reference's int()
    w = tuple(np.abs(v) for v in ((1 - al) * (1 - be), al * (1 - be), (1 - al) * be, al * be))
    pos = ((idx["yT"], idx["xL"]), (idx["yT"], idx["xR"]), (idx["yB"], idx["xL"]), (idx["yB"], idx["xR"]))
    mag, cnt, hit = np.zeros_like(img), np.zeros((B, H, W)), np.zeros((B, H, W))
    neg = rs_negative_sources(r).astype(np.float64)
    for b in range(B):
        for wi, (yy, xx) in zip(w, pos):
            np.add.at(cnt[b], (yy[b], xx[b]), 1.0)
            np.add.at(hit[b], (yy[b], xx[b]), neg[b])
            for c in range(C):
                np.add.at(mag[b, c], (yy[b], xx[b]), wi[b] * g[b, c])
    TL, TR, BL, BR = _taps(img, idx)
    gx, gy = (1 - (yf - fy))[:, None], (1 - (xf - fx))[:, None]
    mx = (gx * g * (TR + TL) + (1 - gx) * g * (BR + BL)).sum(1)
    my = (gy * g * (BL + TL) + (1 - gy) * g * (BR + TR)).sum(1)
    return bound(cnt[:, None], 6, mag), bound(4 * C, 6, np.stack([mx, my], 1)), np.broadcast_to((hit > 0)[:, None], img.shape)


def rs_adjoint(r):
    import torch
    ti = torch.from_numpy(r["img"]).double().requires_grad_()
    tf = torch.from_numpy(r["flow"]).double().requires_grad_()
    ref.resample2d_fwd(ti, tf).backward(torch.from_numpy(r["gout"]).double())
    return ti.grad.numpy(), tf.grad.numpy()


# ---- channelnorm -----------------------------------------------------------------------------------------------------------
def cn_fwd_bound(n):
    """sum of C squares: relative error C u, halved by the square root; extra: the root, the compared value's rounding, second
    order.  inf stays inf (compared separately)."""
    out = n["out"].astype(np.float64)
    return bound(0.5 * n["x"].shape[1], 3, np.where(np.isfinite(out), out, 0.0))


def cn_bwd(n):
    """(float64 restatement of g * x / (out + 1e-9) on the fixture's fp32 out, bound): one term; extra: the fp32 product, the
    fp32 rounding of the quotient, second order."""
    with np.errstate(over="ignore"):
        want = ref.channelnorm_bwd(n["x"].astype(np.float64), n["out"].astype(np.float64), n["gout"].astype(np.float64))
    return want, bound(1, 3, np.abs(want))
