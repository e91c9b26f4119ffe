"""Autograd drop-ins for FlowNet2's three custom operators (training path).

The reference binds Correlation, Resample2d and ChannelNorm as cffi `_ext` modules behind autograd Functions
(networks/*_package/functions/*.py) and nn.Modules (networks/*_package/modules/*.py).  These classes keep the reference's
argument lists and defaults; forward runs ft_*_fwd and backward runs ft_*_bwd (include/flowtrack_hip.h) on the current
stream.  Only the gradients autograd asks for are computed (NULL for the others).  Inputs must be fp32 CUDA tensors; there is
no CPU or half-precision path.  Resample2d's grad of input1 is summed with float atomics, as the reference's: it can differ in
the last bits from run to run; every other gradient is bit-reproducible.

    from flowtrack.pytorch_amd.flownet.ops import Correlation, Resample2d, ChannelNorm
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import FlowtrackHipError, check

__all__ = ["CorrelationFunction", "Resample2dFunction", "ChannelNormFunction", "Correlation", "Resample2d", "ChannelNorm"]


def _fp32_cuda(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        what = f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise FlowtrackHipError(f"{name}: the HIP operators take fp32 CUDA tensors, got {what}")
    if t.dim() != 4:
        raise FlowtrackHipError(f"{name}: expected an NCHW tensor, got shape {tuple(t.shape)}")
    return t.contiguous()


def _stream(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


class CorrelationFunction(Function):
    """correlation_package/functions/correlation.py: same arguments and defaults."""

    @staticmethod
    def forward(ctx, input1, input2, pad_size=3, kernel_size=3, max_displacement=20, stride1=1, stride2=2, corr_multiply=1):
        input1, input2 = _fp32_cuda(input1, "Correlation input1"), _fp32_cuda(input2, "Correlation input2")
        if input1.shape != input2.shape or input1.device != input2.device:
            raise FlowtrackHipError(f"Correlation: inputs differ: {tuple(input1.shape)} vs {tuple(input2.shape)}")
        B, C, H, W = input1.shape
        lib = _lib.load()
        oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib.ft_correlation_out_shape(C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2, ctypes.byref(oc),
                                           ctypes.byref(oh), ctypes.byref(ow)), "Correlation")
        out = torch.empty((B, oc.value, oh.value, ow.value), dtype=torch.float32, device=input1.device)
        with torch.cuda.device(input1.device):
            check(lib.ft_correlation_fwd(_ptr(input1), _ptr(input2), _ptr(out), B, C, H, W, pad_size, kernel_size, max_displacement,
                                         stride1, stride2, corr_multiply, _stream(input1.device)), "ft_correlation_fwd")
        ctx.save_for_backward(input1, input2)
        ctx.params = (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2):
            return (None,) * 8
        grad_output = _fp32_cuda(grad_output, "Correlation grad_output")
        g1 = torch.empty_like(input1) if need1 else None
        g2 = torch.empty_like(input2) if need2 else None
        B, C, H, W = input1.shape
        with torch.cuda.device(input1.device):
            check(_lib.load().ft_correlation_bwd(_ptr(input1), _ptr(input2), _ptr(grad_output), _ptr(g1), _ptr(g2), B, C, H, W,
                                                 *ctx.params, _stream(input1.device)), "ft_correlation_bwd")
        return (g1, g2) + (None,) * 6


class Resample2dFunction(Function):
    """resample2d_package/functions/resample2d.py: same arguments and defaults (kernel_size 1 only, as modules/resample2d.py)."""

    @staticmethod
    def forward(ctx, input1, input2, kernel_size=1):
        if kernel_size != 1:
            raise FlowtrackHipError(f"Resample2d: kernel_size {kernel_size} is not supported (the reference's modules use 1)")
        input1, input2 = _fp32_cuda(input1, "Resample2d input1"), _fp32_cuda(input2, "Resample2d input2")
        B, C, H, W = input1.shape
        if tuple(input2.shape) != (B, 2, H, W) or input1.device != input2.device:
            raise FlowtrackHipError(f"Resample2d: flow of shape {tuple(input2.shape)} for an input of shape {tuple(input1.shape)}")
        out = torch.empty_like(input1)
        with torch.cuda.device(input1.device):
            check(_lib.load().ft_resample2d_fwd(_ptr(input1), _ptr(input2), _ptr(out), B, C, H, W, _stream(input1.device)),
                  "ft_resample2d_fwd")
        ctx.save_for_backward(input1, input2)
        ctx.kernel_size = kernel_size
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2):
            return None, None, None
        grad_output = _fp32_cuda(grad_output, "Resample2d grad_output")
        g1 = torch.empty_like(input1) if need1 else None
        g2 = torch.empty_like(input2) if need2 else None
        B, C, H, W = input1.shape
        with torch.cuda.device(input1.device):
            check(_lib.load().ft_resample2d_bwd(_ptr(input1), _ptr(input2), _ptr(grad_output), _ptr(g1), _ptr(g2), B, C, H, W,
                                                _stream(input1.device)), "ft_resample2d_bwd")
        return g1, g2, None


class ChannelNormFunction(Function):
    """channelnorm_package/functions/channelnorm.py: same arguments and defaults (the L2 norm: norm_deg 2 only)."""

    @staticmethod
    def forward(ctx, input1, norm_deg=2):
        if norm_deg != 2:
            raise FlowtrackHipError(f"ChannelNorm: norm_deg {norm_deg} is not supported (the reference's kernels compute the L2 norm)")
        input1 = _fp32_cuda(input1, "ChannelNorm input1")
        B, C, H, W = input1.shape
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=input1.device)
        with torch.cuda.device(input1.device):
            check(_lib.load().ft_channelnorm_fwd(_ptr(input1), _ptr(out), B, C, H, W, _stream(input1.device)), "ft_channelnorm_fwd")
        ctx.save_for_backward(input1, out)
        ctx.norm_deg = norm_deg
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, out = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        grad_output = _fp32_cuda(grad_output, "ChannelNorm grad_output")
        g1 = torch.empty_like(input1)
        B, C, H, W = input1.shape
        with torch.cuda.device(input1.device):
            check(_lib.load().ft_channelnorm_bwd(_ptr(input1), _ptr(out), _ptr(grad_output), _ptr(g1), B, C, H, W,
                                                 _stream(input1.device)), "ft_channelnorm_bwd")
        return g1, None


class Correlation(nn.Module):
    """correlation_package/modules/correlation.py."""

    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super().__init__()
        self.pad_size = pad_size
        self.kernel_size = kernel_size
        self.max_displacement = max_displacement
        self.stride1 = stride1
        self.stride2 = stride2
        self.corr_multiply = corr_multiply

    def forward(self, input1, input2):
        return CorrelationFunction.apply(input1, input2, self.pad_size, self.kernel_size, self.max_displacement, self.stride1,
                                         self.stride2, self.corr_multiply)


class Resample2d(nn.Module):
    """resample2d_package/modules/resample2d.py."""

    def __init__(self, kernel_size=1):
        super().__init__()
        self.kernel_size = kernel_size

    def forward(self, input1, input2):
        input1_c = input1.contiguous()
        return Resample2dFunction.apply(input1_c, input2, self.kernel_size)


class ChannelNorm(nn.Module):
    """channelnorm_package/modules/channelnorm.py."""

    def __init__(self, norm_deg=2):
        super().__init__()
        self.norm_deg = norm_deg

    def forward(self, input1):
        return ChannelNormFunction.apply(input1, self.norm_deg)
