"""Every kernel form behind ft_correlation_nhwc_fwd against the float64 reference (tests/correlation_ref.py), at the rows of
tests/correlation_cases.py: the VALU kernel (fp16 / fp32), the one-row matrix-core kernel, the three-row kernel and its W <= 64
form.  ft_correlation_nhwc_form pins which of them a row reaches, so a changed dispatch condition fails here instead of silently
turning one form's case into another's.  Every test is a single launch on a map of at most a few thousand pixels; repeated
launches under memory load are test_flow_gpu.py::test_correlation_rows_kernel_is_deterministic_under_memory_load.

Not covered, on purpose: resample2d_pair_kernel (csrc/flow_ops.hip) is reachable only with >= 2 GiB of input or a grid of more
than 2^31 blocks, which no test of a few seconds can build; the same holds for the >= 2 GiB branches of the correlation
dispatch, whose conditions test_correlation_forms_cpu.py::test_form_boundaries pins."""
import ctypes

import pytest
import torch

import correlation_cases as cc
from correlation_ref import activation, correlation_nhwc_ref, error_bound, in_image_mask, worst_ratio

pytestmark = pytest.mark.gpu

ACTS = {"none": (cc.NONE, 0.0), "relu": (cc.RELU, 0.0), "leaky0.1": (cc.LEAKY, 0.1)}
NON_FINITE_ACTS = dict(ACTS, leaky0=(cc.LEAKY, 0.0))      # slope 0: torch's x * negative_slope turns a -inf sum into NaN
WORST = {}        # form -> largest err / bound seen so far in this session (printed, not asserted: the assertion is per case)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _form(hip_lib, c, act, slope):
    return hip_lib.ft_correlation_nhwc_form(c.B, c.C, c.H, c.W, c.d, c.s2, c.f_cstride, c.y_cstride, c.y_coff, act, slope, c.dtype)


def _launch(hip_lib, c, act, slope, f1, f2):
    """One launch on torch's current stream into a sentinel-filled y.  Returns (status, y on the CPU)."""
    g1, g2 = f1.cuda(), f2.cuda()
    y = torch.full((c.B, c.H, c.W, c.y_cstride), cc.SENTINEL, dtype=cc.torch_dtype(c), device="cuda")
    st = hip_lib.ft_correlation_nhwc_fwd(g1.data_ptr(), g2.data_ptr(), y.data_ptr(), c.B, c.C, c.H, c.W, c.d, c.s2, c.f_cstride,
                                         c.y_cstride, c.y_coff, act, slope, c.dtype, _stream())
    torch.cuda.synchronize()
    return st, y.cpu()


def _split(c, y):
    """(the cost-volume slice as float64, True when every channel outside it still holds the sentinel)."""
    dd = cc._dd(c.d, c.s2)
    outside = torch.cat([y[..., :c.y_coff], y[..., c.y_coff + dd:]], -1)
    return y[..., c.y_coff:c.y_coff + dd].double(), bool((outside == cc.SENTINEL).all())


def _check_dense(hip_lib, c, act, slope, label):
    form = _form(hip_lib, c, act, slope)
    assert form == cc.expected_form(c, act, slope)
    f1, f2 = cc.make_features(c)
    st, y = _launch(hip_lib, c, act, slope, f1, f2)
    assert st == 0
    got, untouched = _split(c, y)
    assert untouched, "channels outside [y_coff, y_coff + D*D) were written"
    assert (got != cc.SENTINEL).all(), "cells of the slice were not written"
    assert torch.isfinite(got).all()
    raw, S = cc.reference(c)
    want = activation(raw, act, slope)
    err, bound = (got - want).abs(), error_bound(want, S, c.C, c.dtype == cc.F16)
    ratio = worst_ratio(err, bound)
    at = tuple(int(i) for i in torch.unravel_index(torch.argmax(err - 2 * bound), err.shape))    # (n, y, x, dyi * D + dxi)
    name = cc.FORM_NAMES[form] + ("32" if c.dtype == cc.F32 else "")
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{c.name} {label} -> {name}: max err / bound {ratio:.3f} (worst {name} so far {WORST[name]:.3f})")
    assert ratio <= 2.0, f"worst cell {at}: got {float(got[at])!r}, want {float(want[at])!r}; {int((err > 2 * bound).sum())} of {err.numel()} cells out"
    return got


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_every_form_matches_the_reference(hip_lib, case, act):
    """|got - want| <= 2 * (C 2^-24 S + 2^-23 |want| [+ 2^-11 |want| + 2^-25 for fp16 output]) per element, S = 1/C sum |a b|:
    worst-case fp32 accumulation, the 1/C and slope multiplies, one rounding to fp16; the factor 2 is for the summation order
    inside an MFMA, which the ISA does not document.  NaN in the gap channels of f_cstride > C must stay out, the channels
    around the slice keep their sentinel, every cell of the slice is written."""
    _check_dense(hip_lib, case, *ACTS[act], act)


ONE_PER_FORM = ["rows64_1x4x33_f288", "rows_1x3x65_f288", "mfma_d4_1x5x66_f264", "valu16_c64_d5_s2_2x2x33_f64"]


@pytest.mark.parametrize("slope", [1.5, -0.25])
@pytest.mark.parametrize("name", ONE_PER_FORM)
def test_leaky_slope_outside_0_1(hip_lib, name, slope):
    """act(v) = v > 0 ? v : slope * v for ANY slope.  The two rows kernels compute max(v, slope * v), which is 1.5 v for v > 0
    at slope 1.5: such calls run the one-row kernel (asserted through ft_correlation_nhwc_form in _check_dense)."""
    _check_dense(hip_lib, cc.by_name(name), cc.LEAKY, slope, f"leaky{slope}")


@pytest.mark.parametrize("act", list(NON_FINITE_ACTS))
@pytest.mark.parametrize("name", ONE_PER_FORM + ["valu32_c24_d4_s2_2x2x17_f24"])
def test_non_finite_accumulators(hip_lib, name, act):
    """torch's value for every input: act(NaN) = NaN, act(+inf) = +inf, ReLU(-inf) = 0 exactly, leaky / none(-inf) = -inf,
    and leaky with slope 0 at -inf = NaN (-inf * 0, which is what torch.nn.functional.leaky_relu returns).
    One f1 pixel carries +inf in channel 0 (its cells are +-inf by the sign of f2's channel 0), another NaN in channel 1.  Only
    cells whose f2 pixel lies inside the image are compared: outside, the reference multiplies its zero padding by inf, the
    kernels either do the same or (W <= 64 rows form) write a literal 0."""
    c = cc.by_name(name)
    a, slope = NON_FINITE_ACTS[act]
    assert _form(hip_lib, c, a, slope) == cc.expected_form(c, a, slope)
    f1, f2 = cc.make_features(c)
    lead = f2[..., :2]
    lead[lead == 0] = 1.0
    f1[0, 1, 2, 0] = float("inf")
    f1[0, 0, c.W - 1, 1] = float("nan")
    st, y = _launch(hip_lib, c, a, slope, f1, f2)
    assert st == 0
    got, untouched = _split(c, y)
    assert untouched
    raw, S = correlation_nhwc_ref(f1, f2, c.C, c.d, c.s2, cc.NONE, 0.0)
    want = activation(raw, a, slope)
    m = in_image_mask(c.H, c.W, c.d, c.s2).unsqueeze(0).expand_as(want)
    got, want, raw, S = got[m], want[m], raw[m], S[m]
    neg_inf = torch.isneginf(raw)
    assert torch.isnan(want).any() and torch.isposinf(want).any() and neg_inf.any()      # the case has all three
    bad_nan = int((torch.isnan(got) != torch.isnan(want)).sum())
    bad_pinf = int((torch.isposinf(got) != torch.isposinf(want)).sum())
    at_neg_inf = got[neg_inf]
    print(f"{name} {act}: NaN cells {int(torch.isnan(want).sum())} (mismatched {bad_nan}), +inf cells "
          f"{int(torch.isposinf(want).sum())} (mismatched {bad_pinf}), -inf cells {int(neg_inf.sum())} -> {at_neg_inf.unique().tolist()}")
    assert bad_nan == 0 and bad_pinf == 0
    if a == cc.RELU:
        assert (at_neg_inf == 0).all()
    elif a == cc.LEAKY and slope == 0.0:
        assert torch.isnan(at_neg_inf).all()
    else:
        assert torch.isneginf(at_neg_inf).all()
    fin = torch.isfinite(want)
    ratio = worst_ratio((got[fin] - want[fin]).abs(), error_bound(want[fin], S[fin], c.C, c.dtype == cc.F16))
    print(f"{name} {act}: finite cells max err / bound {ratio:.3f}")
    assert ratio <= 2.0


@pytest.mark.parametrize("case", cc.REFUSED + cc.INVALID, ids=lambda c: c.name)
def test_refusals_leave_y_alone(hip_lib, case):
    c = case
    assert _form(hip_lib, c, cc.LEAKY, 0.1) == -1
    f = torch.zeros((c.B, c.H, c.W, max(c.f_cstride, c.C)), dtype=cc.torch_dtype(c))
    st, y = _launch(hip_lib, c, cc.LEAKY, 0.1, f, f)
    assert st == (cc.UNSUPPORTED if c in cc.REFUSED else cc.INVALID_ARG)
    assert (y == cc.SENTINEL).all()


def test_forms_agree_with_each_other(hip_lib):
    """One feature pair, d 20, [2, 7, 64]: the W <= 64 rows form (8-aligned slice), the 104-column rows form (y_coff 33) and the
    one-row form (reached through ReLU) each within the bound of the reference; their mutual differences are printed."""
    base = cc.Case("agree_2x7x64", cc.ROWS64, cc.F16, 2, 256, 7, 64, 20, 2, 256, 480, 32)
    r64 = _check_dense(hip_lib, base, cc.LEAKY, 0.1, "leaky0.1")
    rows = _check_dense(hip_lib, base._replace(form=cc.ROWS, y_coff=33), cc.LEAKY, 0.1, "leaky0.1")
    one = _check_dense(hip_lib, base, cc.RELU, 0.0, "relu")                               # expected_form: MFMA
    raw, _ = cc.reference(base)
    pos = raw > 0                                                                         # where ReLU and leaky are the same function
    print(f"mutual max |diff|: rows64 vs rows {float((r64 - rows).abs().max()):.3e}, rows64 vs one-row (v > 0) "
          f"{float((r64 - one)[pos].abs().max()):.3e}, rows vs one-row (v > 0) {float((rows - one)[pos].abs().max()):.3e}")
