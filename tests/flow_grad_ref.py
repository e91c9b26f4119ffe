"""float64 restatements of FlowNet2's three custom operators, for the gradient tests.

Two sets:
- differentiable torch restatements of the forwards (the reference's zero padding, nelems, floor / clamp and 1e-9), whose
  autograd is the exact adjoint the HIP backward kernels compute; ChannelNorm's backward is written out, as the reference's;
- direct restatements of the reference's backward loops (correlation_cuda_kernel.cu:108-290, Resample2d_kernel.cu:68-186,
  ChannelNorm_kernel.cu:54-81), vectorised over batch and channels only.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


# ---- differentiable forwards ---------------------------------------------------------------------------------------------
def correlation_fwd(in1, in2, pad, k, md, s1, s2):
    """correlation_cuda_kernel.cu:10-106 on zero-padded inputs: out[n, tj*D+ti, y, x] = 1/(k*k*C) sum_{j,i,c} p1 * p2."""
    B, C, H, W = in1.shape
    krad, drad = (k - 1) // 2, md // s2
    border = krad + md
    p1, p2 = F.pad(in1, (pad,) * 4), F.pad(in2, (pad,) * 4)
    ph, pw = H + 2 * pad, W + 2 * pad
    oh, ow = -(-(ph - 2 * border) // s1), -(-(pw - 2 * border) // s1)
    ys, xs = border + s1 * torch.arange(oh), border + s1 * torch.arange(ow)
    outs = []
    for tj in range(-drad, drad + 1):
        for ti in range(-drad, drad + 1):
            acc = 0
            for j in range(-krad, krad + 1):
                for i in range(-krad, krad + 1):
                    a = p1[:, :, ys + j][:, :, :, xs + i]
                    b = p2[:, :, ys + j + tj * s2][:, :, :, xs + i + ti * s2]
                    acc = acc + (a * b).sum(1)
            outs.append(acc / (k * k * C))
    return torch.stack(outs, 1)


def _coords(flow):
    """x + dx, y + dy rounded to fp32 as the kernels compute them, differentiable in the flow."""
    B, _, H, W = flow.shape
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    out = []
    for base, f in ((xs, flow[:, 0]), (ys, flow[:, 1])):
        exact = base + f
        f32 = (base.float() + f.detach().float()).double()
        out.append(exact + (f32 - exact).detach())
    return out


def resample2d_fwd(img, flow):
    """Resample2d_kernel.cu:20-66: weights from the unclamped floor, neighbour indices clamped, no renormalisation."""
    B, C, H, W = img.shape
    xf, yf = _coords(flow)
    fx, fy = torch.floor(xf).detach(), torch.floor(yf).detach()
    a, b = (xf - fx).unsqueeze(1), (yf - fy).unsqueeze(1)
    xL, xR = fx.clamp(0, W - 1).long(), (fx + 1).clamp(0, W - 1).long()
    yT, yB = fy.clamp(0, H - 1).long(), (fy + 1).clamp(0, H - 1).long()
    flat = img.reshape(B, C, H * W)

    def tap(yy, xx):
        return flat.gather(2, (yy * W + xx).reshape(B, 1, H * W).expand(B, C, H * W)).reshape(B, C, H, W)

    return (1 - a) * (1 - b) * tap(yT, xL) + a * (1 - b) * tap(yT, xR) + (1 - a) * b * tap(yB, xL) + a * b * tap(yB, xR)


class ChannelNormFn(torch.autograd.Function):
    """sqrt(sum_c x^2) with the reference's backward g * x / (out + 1e-9) (0 at a zero vector, where autograd of sqrt is NaN)."""

    @staticmethod
    def forward(ctx, x):
        out = torch.sqrt((x * x).sum(1, keepdim=True))
        ctx.save_for_backward(x, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, out = ctx.saved_tensors
        return channelnorm_bwd(x, out, g)


def channelnorm_fwd(x):
    return ChannelNormFn.apply(x)


def channelnorm_bwd(x, out, g):
    return g * x / (out + 1e-9)


# ---- the reference's backward loops -------------------------------------------------------------------------------------
def _cdiv(a: int, b: int) -> int:
    """C integer division (truncates toward zero)."""
    q = abs(a) // b
    return q if a >= 0 else -q


def correlation_bwd_loops(in1, in2, g, pad, k, md, s1, s2):
    """Correlation_backward_input1 / _input2 (correlation_cuda_kernel.cu:108-290) over padded NHWC copies; numpy float64.
    For stride1 > 1 only the blocks whose pixel (yi * stride1, xi * stride1) lies inside the map are restated: the reference's
    other blocks write through the flat index into the next row / channel or past the tensor (flowops_pinned.corr_stray_targets,
    shown on the reference's own numbers by test_flowops_pinned_cpu.py)."""
    in1, in2, g = (np.asarray(t, dtype=np.float64) for t in (in1, in2, g))
    B, C, H, W = in1.shape
    _, OC, oh, ow = g.shape
    krad, drad = (k - 1) // 2, md // s2
    D = 2 * drad + 1
    r1 = np.pad(in1, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    r2 = np.pad(in2, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    ph, pw = H + 2 * pad, W + 2 * pad
    nelems = k * k * C
    gi1, gi2 = np.zeros_like(in1), np.zeros_like(in2)

    def val(r, yy, xx):
        return r[:, :, yy, xx] if 0 <= yy < ph and 0 <= xx < pw else 0.0

    for yi in range(H):
        for xi in range(W):
            y, x = yi * s1 + pad, xi * s1 + pad
            if yi * s1 >= H or xi * s1 >= W:
                continue
            # input1
            xmin, ymin = _cdiv(x - krad - md, s1), _cdiv(y - krad - md, s1)
            xmax, ymax = _cdiv(x + krad - md, s1), _cdiv(y + krad - md, s1)
            if not (xmax < 0 or ymax < 0 or xmin >= ow or ymin >= oh or xmin > xmax or ymin > ymax):
                xmin, xmax, ymin, ymax = max(0, xmin), min(ow - 1, xmax), max(0, ymin), min(oh - 1, ymax)
                acc = 0.0
                for tc in range(OC):
                    i2, j2 = (tc % D - drad) * s2, (tc // D - drad) * s2
                    gs = g[:, tc, ymin:ymax + 1, xmin:xmax + 1].sum(axis=(1, 2))[:, None]
                    acc = acc + gs * val(r2, y + j2, x + i2)
                gi1[:, :, yi * s1, xi * s1] = acc / nelems
            # input2
            acc = 0.0
            for tc in range(OC):
                i2, j2 = (tc % D - drad) * s2, (tc // D - drad) * s2
                xmin, ymin = _cdiv(x - krad - md - i2, s1), _cdiv(y - krad - md - j2, s1)
                xmax, ymax = _cdiv(x + krad - md - i2, s1), _cdiv(y + krad - md - j2, s1)
                if xmax < 0 or ymax < 0 or xmin >= ow or ymin >= oh or xmin > xmax or ymin > ymax:
                    continue
                xmin, xmax, ymin, ymax = max(0, xmin), min(ow - 1, xmax), max(0, ymin), min(oh - 1, ymax)
                gs = g[:, tc, ymin:ymax + 1, xmin:xmax + 1].sum(axis=(1, 2))[:, None]
                acc = acc + gs * val(r1, y - j2, x - i2)
            gi2[:, :, yi * s1, xi * s1] = acc / nelems
    return gi1, gi2


def resample2d_bwd_loops(img, flow, g):
    """kernel_Resample2d_backward_input1 / _input2 (Resample2d_kernel.cu:68-186), kernel_size 1; numpy float64 with the
    coordinates rounded to fp32 as the kernel computes them."""
    img, g = np.asarray(img, dtype=np.float64), np.asarray(g, dtype=np.float64)
    flow32 = np.asarray(flow, dtype=np.float32)
    B, C, H, W = img.shape
    xf = (np.arange(W, dtype=np.float32)[None, None, :] + flow32[:, 0]).astype(np.float64)
    yf = (np.arange(H, dtype=np.float32)[None, :, None] + flow32[:, 1]).astype(np.float64)
    alpha, beta = xf - np.trunc(xf), yf - np.trunc(yf)           # the reference's int() here; floor in its forward
    fx, fy = np.floor(xf), np.floor(yf)
    xL, xR = np.clip(fx, 0, W - 1).astype(np.int64), np.clip(fx + 1, 0, W - 1).astype(np.int64)
    yT, yB = np.clip(fy, 0, H - 1).astype(np.int64), np.clip(fy + 1, 0, H - 1).astype(np.int64)
    gi = np.zeros_like(img)
    for b in range(B):
        for c in range(C):
            gc, plane = g[b, c], gi[b, c]
            np.add.at(plane, (yT[b], xL[b]), (1 - alpha[b]) * (1 - beta[b]) * gc)
            np.add.at(plane, (yT[b], xR[b]), alpha[b] * (1 - beta[b]) * gc)
            np.add.at(plane, (yB[b], xL[b]), (1 - alpha[b]) * beta[b] * gc)
            np.add.at(plane, (yB[b], xR[b]), alpha[b] * beta[b] * gc)
    bi = np.arange(B)[:, None, None, None]
    ci = np.arange(C)[None, :, None, None]

    def tap(yy, xx):
        return img[bi, ci, yy[:, None], xx[:, None]]

    TL, TR, BL, BR = tap(yT, xL), tap(yT, xR), tap(yB, xL), tap(yB, xR)
    gx = (1 - (yf - fy))[:, None]
    gy = (1 - (xf - fx))[:, None]
    dfx = (gx * g * TR - gx * g * TL + (1 - gx) * g * BR - (1 - gx) * g * BL).sum(1)
    dfy = (gy * g * BL - gy * g * TL + (1 - gy) * g * BR - (1 - gy) * g * TR).sum(1)
    return gi, np.stack([dfx, dfy], 1)
