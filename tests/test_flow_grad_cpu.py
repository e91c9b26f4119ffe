"""Backward of Correlation / Resample2d / ChannelNorm, host side: the float64 restatements (tests/flow_grad_ref.py) against each
other, the argument checks of the ft_*_bwd entry points, and the input checks of flownet.ops.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import flow_grad_ref as ref
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from flowtrack.pytorch_amd.flownet import ops


def _autograd_corr(a, b, g, pad, k, md, s1, s2):
    ta = torch.from_numpy(a).double().requires_grad_()
    tb = torch.from_numpy(b).double().requires_grad_()
    out = ref.correlation_fwd(ta, tb, pad, k, md, s1, s2)
    assert out.shape == g.shape
    out.backward(torch.from_numpy(g).double())
    return ta.grad.numpy(), tb.grad.numpy()


def _corr_inputs(tag, B, C, H, W, pad, k, md, s1, s2):
    a = synth.normal(11, f"ga{tag}", (B, C, H, W)).numpy()
    b = synth.normal(11, f"gb{tag}", (B, C, H, W)).numpy()
    with torch.no_grad():
        shape = ref.correlation_fwd(torch.from_numpy(a), torch.from_numpy(b), pad, k, md, s1, s2).shape
    g = synth.normal(11, f"gg{tag}", tuple(shape)).numpy()
    return a, b, g


# B, C, H, W, pad, k, max_disp, s1, s2 with kernel 1 / stride1 1: pad = md, pad < md, pad > md, stride2 1 and 2
K1_CASES = [(1, 3, 7, 8, 4, 1, 4, 1, 2), (2, 2, 7, 8, 2, 1, 4, 1, 2), (1, 3, 6, 9, 1, 1, 3, 1, 1), (1, 2, 6, 7, 3, 1, 2, 1, 1),
            (1, 2, 5, 6, 0, 1, 2, 1, 2)]


@pytest.mark.parametrize("case", K1_CASES, ids=[str(c) for c in K1_CASES])
def test_correlation_adjoint_equals_reference_loops_k1(case):
    a, b, g = _corr_inputs(str(case), *case)
    want1, want2 = ref.correlation_bwd_loops(a, b, g, *case[4:])
    got1, got2 = _autograd_corr(a, b, g, *case[4:])
    assert np.abs(got1 - want1).max() <= 1e-12 * max(1.0, np.abs(want1).max())
    assert np.abs(got2 - want2).max() <= 1e-12 * max(1.0, np.abs(want2).max())


def test_correlation_reference_is_not_the_adjoint_for_kernel_3():
    """correlation_cuda_kernel.cu's input1 gradient sums the output window [p-krad-md, p+krad-md] while the forward reads
    in1 at [p-2krad-md, p-md]: for kernel_size > 1 the reference is not the gradient of its own forward."""
    case = (1, 3, 9, 10, 3, 3, 2, 1, 1)
    a, b, g = _corr_inputs("k3", *case)
    want1, want2 = ref.correlation_bwd_loops(a, b, g, *case[4:])
    got1, got2 = _autograd_corr(a, b, g, *case[4:])
    assert np.abs(got1 - want1).max() > 1e-2 * np.abs(got1).max()


def test_resample2d_adjoint_equals_reference_loops():
    B, C, H, W = 2, 3, 7, 8
    img = synth.normal(12, "rimg", (B, C, H, W)).numpy()
    flow = (synth.uniform(12, "rflow", (B, 2, H, W), -12.0, 12.0)).numpy()      # taps up to 12 px outside the 7 x 8 image
    flow[0, :, 0, 0] = (1e9, -1e9)
    flow[1, :, 2, 3] = (0.0, 0.0)
    flow[1, :, 4, 5] = (-3.0, 2.0)                                              # integer coordinates
    g = synth.normal(12, "rg", (B, C, H, W)).numpy()
    ti = torch.from_numpy(img).double().requires_grad_()
    tf = torch.from_numpy(flow).double().requires_grad_()
    ref.resample2d_fwd(ti, tf).backward(torch.from_numpy(g).double())
    want_i, want_f = ref.resample2d_bwd_loops(img, flow, g)
    assert np.isfinite(want_f).all()
    assert np.abs(ti.grad.numpy() - want_i).max() <= 1e-12
    assert np.abs(tf.grad.numpy() - want_f).max() <= 1e-12


def test_channelnorm_backward_formula():
    x = synth.normal(13, "cn", (2, 3, 4, 5)).double()
    x[0, :, 1, 1] = 0.0                                                          # zero vector: gradient 0, not NaN
    g = synth.normal(13, "cng", (2, 1, 4, 5)).double()
    xr = x.clone().requires_grad_()
    ref.channelnorm_fwd(xr).backward(g)
    assert torch.isfinite(xr.grad).all() and float(xr.grad[0, :, 1, 1].abs().max()) == 0.0
    xa = x.clone().requires_grad_()
    torch.sqrt((xa * xa).sum(1, keepdim=True)).backward(g)                      # autograd of sqrt, away from the zero vector
    mask = torch.ones_like(x, dtype=torch.bool)
    mask[0, :, 1, 1] = False
    assert torch.allclose(xr.grad[mask], xa.grad[mask], rtol=1e-7, atol=1e-12)


def test_backward_entry_points_check_arguments(hip_lib):
    p = ctypes.c_void_p(16)                     # never dereferenced: every call below must fail its checks before any launch
    null = ctypes.c_void_p(None)
    s = ctypes.c_void_p(None)
    INV, UNS = _lib.FT_ERR_INVALID_ARG, _lib.FT_ERR_UNSUPPORTED
    corr = hip_lib.ft_correlation_bwd
    assert corr(null, p, p, p, p, 1, 8, 8, 8, 4, 1, 4, 1, 2, 1, s) == INV             # NULL input
    assert corr(p, p, null, p, p, 1, 8, 8, 8, 4, 1, 4, 1, 2, 1, s) == INV             # NULL grad_out
    assert corr(p, p, p, null, null, 1, 8, 8, 8, 4, 1, 4, 1, 2, 1, s) == INV          # both gradients NULL
    assert corr(p, p, p, p, p, 1, 8, 8, 8, 4, 1, 4, 1, 2, 2, s) == UNS                # corr_type_multiply 2
    assert corr(p, p, p, p, p, 1, 8, 8, 8, 0, 1, 20, 1, 2, 1, s) == INV               # no output pixel
    assert corr(p, p, p, p, p, 1, 8, 8, 8, 4, 0, 4, 1, 2, 1, s) == INV                # kernel_size 0
    assert corr(p, p, p, p, p, 0, 8, 8, 8, 4, 1, 4, 1, 2, 1, s) == INV                # B 0
    rs = hip_lib.ft_resample2d_bwd
    assert rs(null, p, p, p, p, 1, 3, 8, 8, s) == INV
    assert rs(p, p, null, p, p, 1, 3, 8, 8, s) == INV
    assert rs(p, p, p, null, null, 1, 3, 8, 8, s) == INV
    assert rs(p, p, p, p, p, 1, 0, 8, 8, s) == INV
    cn = hip_lib.ft_channelnorm_bwd
    assert cn(p, p, p, null, 1, 3, 8, 8, s) == INV
    assert cn(p, null, p, p, 1, 3, 8, 8, s) == INV
    assert cn(p, p, p, p, 1, 3, 0, 8, s) == INV


@pytest.mark.parametrize("dtype,device", [(torch.float16, "cpu"), (torch.float32, "cpu"), (torch.float64, "cpu")])
def test_ops_reject_non_fp32_cuda_tensors(dtype, device):
    x = torch.zeros((1, 3, 8, 8), dtype=dtype, device=device)
    flow = torch.zeros((1, 2, 8, 8), dtype=dtype, device=device)
    with pytest.raises(FlowtrackHipError):
        ops.Correlation(4, 1, 4, 1, 2, 1)(x, x)
    with pytest.raises(FlowtrackHipError):
        ops.Resample2d()(x, flow)
    with pytest.raises(FlowtrackHipError):
        ops.ChannelNorm()(x)


def test_ops_signatures_match_the_reference():
    import inspect

    assert str(inspect.signature(ops.CorrelationFunction.forward)) == (
        "(ctx, input1, input2, pad_size=3, kernel_size=3, max_displacement=20, stride1=1, stride2=2, corr_multiply=1)")
    assert str(inspect.signature(ops.Resample2dFunction.forward)) == "(ctx, input1, input2, kernel_size=1)"
    assert str(inspect.signature(ops.ChannelNormFunction.forward)) == "(ctx, input1, norm_deg=2)"
    assert str(inspect.signature(ops.Correlation.__init__)) == (
        "(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1)")
    assert str(inspect.signature(ops.Resample2d.__init__)) == "(self, kernel_size=1)"
    assert str(inspect.signature(ops.ChannelNorm.__init__)) == "(self, norm_deg=2)"
