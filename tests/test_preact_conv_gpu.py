"""ft_preact_conv1x1_fwd (include/flowtrack_hip.h) alone, through the C ABI, fp16 and fp32: the 1x1 conv of a DenseNet layer /
transition whose input goes through BatchNorm + ReLU (+ the 2x2 average pool) on its way into the GEMM.

  * every row of fpn_densenet_ref.PREACT_CASES within the derived bound of the float64 restatement (preact_conv1x1_ref), with the
    channels of x past Cin filled with NaN wherever the buffer has any (the loader must mask them, not multiply them by zero
    weights) and the channels of y outside the written window checked untouched;
  * integer-exact variants of rows b and d (exact_preact_cases.py) bit for bit;
  * pool = 0, no activation, identity epilogue against ft_scale_shift_act_nhwc_fwd + ft_conv2d_fwd (hip_ops.PreactConv1x1's two
    forms) within the sum of the two kernels' bounds around the exact sum of the operands both read;
  * refusals return their codes and leave a sentinel-filled y untouched.
Shapes: the smallest that reach each path — one pixel and half a K chunk; a masked K tail with a pixel count off any tile; K = 1056
on 12 pixels (the 1-wave workgroups of the late blocks); odd maps under the pool; and the two 32768-pixel rows at which the fp16
dispatch switches to the 4-wave 128-pixel x 128-output workgroups (the shape of dense blocks 1 and 2).

Measured on an MI355X, worst error / derived bound over all elements of a row: fp16 0.12 (c) .. 0.42 (f, g), fp32 0.003 (c) .. 0.08 (g);
fused against the two-launch form 0.92 of the summed bounds at most (f, fp16), against the exact sum of its own operands 0.98 (f, fp16:
that bound is K u S + one fp16 rounding, no slack in it); the integer-exact rows bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import fpn_densenet_ref as dref
from exact_preact_cases import exact_case, exact_want
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd.hip_ops import ActView, PreactConv1x1, current_stream_handle, pack_preact_weights
from util import make_program, run_program

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
SENTINEL = 7.25
CASES = {c[0][0]: c for c in dref.PREACT_CASES}


def _ptr(t):
    return t.data_ptr() if torch.is_tensor(t) else t


def _call(lib, x, w, ps, pb, qs, qb, y, dtype, N, H, W, cin, xcs, xoff, cout, ycs, yoff, pool, act):
    st = lib.ft_preact_conv1x1_fwd(_ptr(x), _ptr(w), _ptr(ps), _ptr(pb), _ptr(qs), _ptr(qb), _ptr(y), dtype if isinstance(dtype, int) else _lib.dtype_code(dtype),
                                   N, H, W, cin, xcs, xoff, cout, ycs, yoff, int(pool), act, current_stream_handle(DEV))
    torch.cuda.synchronize()
    return st


def _launch(lib, dtype, x, w, ps, pb, qs, qb, xcs, cout, ycs, yoff, pool, relu):
    """x [N,H,W,Cin] float64 values of `dtype` -> (y window as float64 on the CPU, the whole y buffer); channels [Cin, xcs) of x are NaN."""
    N, H, W, cin = x.shape
    xb = torch.full((N, H, W, xcs), float("nan"), dtype=dtype, device=DEV)
    xb[..., :cin] = x.to(device=DEV, dtype=dtype)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    yb = torch.full((N, Ho, Wo, ycs), SENTINEL, dtype=dtype, device=DEV)
    dev = [None if t is None else t.to(device=DEV, dtype=F32).contiguous() for t in (ps, pb, qs, qb)]
    wp = pack_preact_weights(w, dtype, DEV)
    st = _call(lib, xb, wp, dev[0], dev[1], dev[2], dev[3], yb, dtype, N, H, W, cin, xcs, 0, cout, ycs, yoff, pool,
               _lib.FT_ACT_RELU if relu else _lib.FT_ACT_NONE)
    assert st == _lib.FT_OK, st
    return yb[..., yoff:yoff + cout].double().cpu(), yb.cpu()


def _untouched(yb, yoff, cout):
    return bool((yb[..., :yoff] == SENTINEL).all()) and bool((yb[..., yoff + cout:] == SENTINEL).all())


def _random_case(case, dtype):
    name, N, H, W, cin, xcs, cout, ycs, yoff, pool = case
    x = synth.normal(71, name + ".x", (N, H, W, cin)).to(dtype).double()            # the values the kernel reads
    w = synth.normal(71, name + ".w", (cout, cin), std=cin ** -0.5)
    ps, pb = synth.uniform(71, name + ".ps", (cin,), 0.5, 1.5), synth.normal(71, name + ".pb", (cin,), std=0.3)
    qs, qb = synth.uniform(71, name + ".qs", (cout,), 0.5, 1.5), synth.normal(71, name + ".qb", (cout,), std=0.3)
    return x, w, ps, pb, qs, qb


@DTYPES
@pytest.mark.parametrize("case", dref.PREACT_CASES, ids=lambda c: c[0])
def test_within_derived_bound(hip_lib, case, dtype):
    name, N, H, W, cin, xcs, cout, ycs, yoff, pool = case
    x, w, ps, pb, qs, qb = _random_case(case, dtype)
    relu = not pool                                  # (a dense layer carries norm2 + ReLU behind it, a transition nothing)
    post = (qs, qb) if relu else (None, None)
    got, yb = _launch(hip_lib, dtype, x, w, ps, pb, post[0], post[1], xcs, cout, ycs, yoff, pool, relu)
    want, bound = dref.preact_conv1x1_ref(x, w, ps, pb, post[0], post[1], pool=pool, relu=relu, fp16=dtype == F16)
    err = (got - want).abs()
    ratio = (err / bound).max().item()
    print(f"{name} {dtype}: {tuple(want.shape)} max abs err {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all())
    assert ratio <= 1.0
    assert _untouched(yb, yoff, cout)


@DTYPES
@pytest.mark.parametrize("key", ["b", "d"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "none"])
def test_integer_exact(hip_lib, key, dtype, relu):
    name, N, H, W, cin, xcs, cout, ycs, yoff, pool = CASES[key]
    c = exact_case(name, N, H, W, cin, cout, pool)
    got, yb = _launch(hip_lib, dtype, c["x"], c["w"], c["pre_scale"], c["pre_shift"], c["post_scale"], c["post_shift"], xcs, cout, ycs, yoff, pool, relu)
    want = exact_want(c, pool, relu).numpy().astype(np.float16 if dtype == F16 else np.float32).astype(np.float64)
    assert np.array_equal(got.numpy(), want)
    assert _untouched(yb, yoff, cout)


@DTYPES
@pytest.mark.parametrize("key", ["b", "c", "f"])
def test_matches_two_launch_form(hip_lib, key, dtype):
    """pool = 0, no activation, identity epilogue: the fused launch against ft_scale_shift_act_nhwc_fwd + ft_conv2d_fwd.  Both read
    the same operands bit for bit (the activated copy `a` the first launch writes is the fused kernel's operand by contract, the
    weights round to the same dtype), so with exact = sum_c a_c w_c in float64 each result is within its own accumulation + store
    bound of `exact`: K u S (doubled for the conv: conv_bound.py) + one rounding to the output type each."""
    name, N, H, W, cin, xcs, cout, ycs, yoff, pool = CASES[key]
    x, w, ps, pb, _, _ = _random_case(CASES[key], dtype)
    bn = {"weight": ps, "bias": pb, "running_mean": torch.zeros(cin), "running_var": torch.ones(cin), "eps": 0.0}
    pc = PreactConv1x1(w.reshape(cout, cin, 1, 1), bn, dtype=dtype, device=DEV, label=name)
    xb = torch.full((N, H, W, xcs), float("nan"), dtype=dtype, device=DEV)
    xb[..., :cin] = x.to(device=DEV, dtype=dtype)
    xin = ActView(xb, cin, 0)
    y1, y2 = (ActView(torch.full((N, H, W, ycs), SENTINEL, dtype=dtype, device=DEV), cout, yoff) for _ in range(2))
    a = ActView(torch.zeros((N, H, W, cin), dtype=dtype, device=DEV), cin, 0)
    prog = make_program()
    pc.record(prog, xin, y1)
    pc.record_unfused(prog, xin, y2, a)
    run_program(prog)
    names = [c[0] for c in prog.calls]
    assert names.count("ft_preact_conv1x1_fwd") == 1 and "ft_scale_shift_act_nhwc_fwd" in names
    fused, two = (v.t[..., yoff:yoff + cout].double().cpu() for v in (y1, y2))
    ad, wd = a.t.double().cpu(), w.to(dtype).double()
    exact, S = ad @ wd.t(), ad @ wd.abs().t()
    u, out = 2.0 ** -24, (2.0 ** -11 if dtype == F16 else 2.0 ** -24)
    bound = 3 * cin * u * S + 2 * (out * exact.abs() + 2.0 ** -25) + 4 * u * exact.abs()
    ratio = ((fused - two).abs() / bound.clamp_min(1e-300)).max().item()
    r1 = ((fused - exact).abs() / (cin * u * S + out * exact.abs() + 2.0 ** -25)).max().item()
    print(f"{name} {dtype}: fused vs two launches, worst difference / summed bounds {ratio:.3f}; fused vs the exact sum of its operands {r1:.3f}")
    assert ratio <= 1.0 and r1 <= 1.0
    assert _untouched(y1.t.cpu(), yoff, cout) and _untouched(y2.t.cpu(), yoff, cout)


def test_refusals_launch_nothing(hip_lib):
    lib = hip_lib
    N, H, W, cin, cout = 1, 4, 4, 64, 32
    x = torch.zeros((N, H, W, cin), dtype=F16, device=DEV)
    w = pack_preact_weights(torch.zeros(cout, cin), F16, DEV)
    ps, pb = torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV)
    qs, qb = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    y = torch.full((N, H, W, 64), SENTINEL, dtype=F16, device=DEV)
    ok = dict(x=x, w=w, ps=ps, pb=pb, qs=qs, qb=qb, y=y, dtype=F16, N=N, H=H, W=W, cin=cin, xcs=cin, xoff=0, cout=cout, ycs=64, yoff=0, pool=0,
              act=_lib.FT_ACT_RELU)
    UNS, INV = _lib.FT_ERR_UNSUPPORTED, _lib.FT_ERR_INVALID_ARG
    bad = [
        (UNS, dict(cout=48)), (UNS, dict(cin=60)), (UNS, dict(xoff=4, xcs=72)), (UNS, dict(yoff=4)), (UNS, dict(xcs=68)), (UNS, dict(ycs=68)),
        (UNS, dict(pool=1, H=1)), (UNS, dict(pool=1, W=1)), (UNS, dict(dtype=F32, cin=62)),
        (INV, dict(x=None)), (INV, dict(w=None)), (INV, dict(ps=None)), (INV, dict(pb=None)), (INV, dict(y=None)), (INV, dict(qs=None)), (INV, dict(qb=None)),
        (INV, dict(N=0)), (INV, dict(H=0)), (INV, dict(W=-1)), (INV, dict(cin=0)), (INV, dict(cout=0)), (INV, dict(xcs=56)), (INV, dict(ycs=24)),
        (INV, dict(yoff=40)), (INV, dict(xoff=-8)), (INV, dict(dtype=2)), (INV, dict(act=_lib.FT_ACT_LEAKY)), (INV, dict(act=7)), (INV, dict(pool=2)),
    ]
    for want, change in bad:
        args = dict(ok, **change)
        assert _call(lib, **args) == want, change
        assert bool((y == SENTINEL).all()), change
    assert _call(lib, **ok) == _lib.FT_OK and bool((y[..., :cout] == 0).all()) and bool((y[..., cout:] == SENTINEL).all())
    # identity epilogue: both post_* NULL
    y.fill_(SENTINEL)
    assert _call(lib, **dict(ok, qs=None, qb=None)) == _lib.FT_OK and bool((y[..., :cout] == 0).all())
