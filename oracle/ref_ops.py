"""ORACLE — TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

ctypes calls of the REFERENCE's own host launchers for Correlation / Resample2d / ChannelNorm, forward and backward, in
oracle/_ref/libflowtrack_ref_ops.so — the reference's .cu files compiled for the CPU by oracle/cuda_on_cpu/build_ref.py.
Buffers are allocated as the reference's .c / .py wrappers allocate them: rInput1 / rInput2 [B, H+2p, W+2p, C] zero-filled,
outputs and every gradient zero-filled.  available() tells whether the library exists; nothing here builds it.

Correlation's backward kernels write gradInput at row blockIdx.x * stride1, column blockIdx.y * stride1 for every block of an
[H, W, C] grid, which for stride1 > 1 lies past the tensor (in the reference, past its allocation).  The gradient buffers here
carry stride1 * H * W floats of slack behind them so that those writes stay inside memory we own; the slack is dropped.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from oracle.cuda_on_cpu import build_ref

LIB, LIB_FMA = build_ref.LIB, build_ref.LIB_FMA
_libs = {}


class _Tensor(ctypes.Structure):      # oracle/cuda_on_cpu/THC.h: THCudaTensor
    _fields_ = [("size", ctypes.c_long * 4), ("stride", ctypes.c_long * 4), ("data", ctypes.c_void_p)]


def available() -> bool:
    return os.path.exists(LIB)


def fma_available() -> bool:
    return os.path.exists(LIB_FMA)


def _lib(fma=False):
    path = LIB_FMA if fma else LIB
    if path not in _libs:
        lib = ctypes.CDLL(path)
        lib.Correlation_forward_cuda_kernel.restype = ctypes.c_int
        lib.Correlation_backward_cuda_kernel.restype = ctypes.c_int
        for name in ("Resample2d_kernel_forward", "Resample2d_kernel_backward", "ChannelNorm_kernel_forward",
                     "ChannelNorm_kernel_backward"):
            getattr(lib, name).restype = None
        _libs[path] = lib
    return _libs[path]


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 4
    return a


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _strides(a):
    return [s // a.itemsize for s in a.strides]


def _t(a):
    return ctypes.byref(_Tensor((ctypes.c_long * 4)(*a.shape), (ctypes.c_long * 4)(*_strides(a)), a.ctypes.data))


def correlation_out_shape(C, H, W, pad, k, md, s1, s2):
    """correlation_cuda.c: nOutputChannels, ceil((float)(padded - 2 * border) / (float)stride1)."""
    border = (k - 1) // 2 + md
    D = 2 * (md // s2) + 1
    oh = int(np.ceil(np.float32(H + 2 * pad - 2 * border) / np.float32(s1)))
    ow = int(np.ceil(np.float32(W + 2 * pad - 2 * border) / np.float32(s1)))
    return D * D, oh, ow


def correlation_fwd(in1, in2, pad=20, k=1, md=20, s1=1, s2=2, fma=False):
    in1, in2 = _f32(in1), _f32(in2)
    B, C, H, W = in1.shape
    assert in2.shape == in1.shape
    oc, oh, ow = correlation_out_shape(C, H, W, pad, k, md, s1, s2)
    assert oh > 0 and ow > 0
    out = np.zeros((B, oc, oh, ow), dtype=np.float32)
    r1 = np.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=np.float32)
    r2 = np.zeros_like(r1)
    ok = _lib(fma).Correlation_forward_cuda_kernel(
        _p(out), B, oc, oh, ow, *_strides(out),
        _p(in1), C, H, W, *_strides(in1),
        _p(in2), C, *_strides(in2),
        _p(r1), _p(r2), pad, k, md, s1, s2, 1, None)
    assert ok == 1
    return out


def correlation_bwd(in1, in2, grad_out, pad=20, k=1, md=20, s1=1, s2=2, fma=False):
    in1, in2, g = _f32(in1), _f32(in2), _f32(grad_out)
    B, C, H, W = in1.shape
    oc, oh, ow = correlation_out_shape(C, H, W, pad, k, md, s1, s2)
    assert g.shape == (B, oc, oh, ow)
    r1 = np.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=np.float32)
    r2 = np.zeros_like(r1)
    n = B * C * H * W
    slack = s1 * H * W if s1 > 1 else 0
    buf1, buf2 = np.zeros(n + slack, dtype=np.float32), np.zeros(n + slack, dtype=np.float32)
    gi1, gi2 = buf1[:n].reshape(B, C, H, W), buf2[:n].reshape(B, C, H, W)
    ok = _lib(fma).Correlation_backward_cuda_kernel(
        _p(g), B, oc, oh, ow, *_strides(g),
        _p(in1), C, H, W, *_strides(in1),
        _p(in2), *_strides(in2),
        _p(gi1), *_strides(gi1),
        _p(gi2), C, *_strides(gi2),
        _p(r1), _p(r2), pad, k, md, s1, s2, 1, None)
    assert ok == 1
    return gi1.copy(), gi2.copy()


def resample2d_fwd(img, flow, kernel_size=1, fma=False):
    img, flow = _f32(img), _f32(flow)
    out = np.zeros((img.shape[0], img.shape[1], flow.shape[2], flow.shape[3]), dtype=np.float32)
    _lib(fma).Resample2d_kernel_forward(None, _t(img), _t(flow), _t(out), kernel_size)
    return out


def resample2d_bwd(img, flow, grad_out, kernel_size=1, fma=False):
    img, flow, g = _f32(img), _f32(flow), _f32(grad_out)
    gi1, gi2 = np.zeros_like(img), np.zeros_like(flow)
    _lib(fma).Resample2d_kernel_backward(None, _t(img), _t(flow), _t(g), _t(gi1), _t(gi2), kernel_size)
    return gi1, gi2


def channelnorm_fwd(x, norm_deg=2, fma=False):
    x = _f32(x)
    B, _, H, W = x.shape
    out = np.zeros((B, 1, H, W), dtype=np.float32)
    _lib(fma).ChannelNorm_kernel_forward(None, _t(x), _t(out), norm_deg)
    return out


def channelnorm_bwd(x, out, grad_out, norm_deg=2, fma=False):
    x, out, g = _f32(x), _f32(out), _f32(grad_out)
    gi = np.zeros_like(x)
    _lib(fma).ChannelNorm_kernel_backward(None, _t(x), _t(out), _t(g), _t(gi), norm_deg)
    return gi
