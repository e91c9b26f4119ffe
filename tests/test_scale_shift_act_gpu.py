"""ft_scale_shift_act_nhwc_fwd (include/flowtrack_hip.h): y[pix, c] = act(scale[c] * x[pix, c] + shift[c]) on NHWC views, the
pre-activation BatchNorm + ReLU in front of the lateral-deconv head's first deconv.

The stated arithmetic, restated in numpy: v = fma(scale, x, shift) in fp32 (evaluated in float64 and rounded once to fp32), then
act_mul's rules (v > 0 -> v, NaN -> NaN, else k * v with 0 * anything = 0: ReLU(-inf) = 0, none(-inf) = leaky(-inf) = -inf), then one
rounding to the output type.
  * bit for bit on data where a fused and an unfused multiply-add coincide (small integers, power-of-two scales, (half-)integer shifts);
  * within 1 ulp of the output type of the float64 value on random data (the fp32 multiply-add contributes half an fp32 ulp, the store
    half an ulp of the output type: together under one ulp of either type);
  * channels outside the written slice keep their NaN guard; C = 8, 24, 2048 at 1, 7 and 144 pixels, slices with coff != 0 and
    cstride > C, both dtypes, all three activations; a view that is not 16-byte aligned (the element-wise form); in place; more
    (pixel, group) items than one pass of the capped grid (2048 workgroups of 256 threads)."""
import ctypes

import pytest
import torch

from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd.hip_ops import ActView, current_stream_handle, record_scale_shift_act
from util import make_program, run_program

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
NAN = float("nan")
SLOPE = 0.25
ACTS = (("none", _lib.FT_ACT_NONE, 1.0), ("relu", _lib.FT_ACT_RELU, 0.0), ("leaky", _lib.FT_ACT_LEAKY, SLOPE))
MAX_BLOCKS = 2048          # the kernel's grid cap (csrc/posenet_ops.hip)


def _call(lib, x, y, dtype, npix, C, xcs, xoff, ycs, yoff, scale, shift, act, slope=SLOPE):
    return lib.ft_scale_shift_act_nhwc_fwd(x.data_ptr() if torch.is_tensor(x) else x, y.data_ptr() if torch.is_tensor(y) else y, _lib.dtype_code(dtype),
                                           ctypes.c_longlong(npix), C, xcs, xoff, ycs, yoff, scale.data_ptr() if torch.is_tensor(scale) else scale,
                                           shift.data_ptr() if torch.is_tensor(shift) else shift, act, ctypes.c_float(slope), current_stream_handle(DEV))


def _ref(x64, scale, shift, k):
    """float64 -> (the stated arithmetic's fp32 value before the store, the exact float64 value)."""
    exact = scale.double() * x64 + shift.double()

    def act(v):
        t = torch.zeros_like(v) if k == 0 else v * k          # (the legacy multiply: 0 * anything = 0)
        return torch.where(torch.isnan(v), v, torch.where(v > 0, v, t))
    return act(exact.float().double()), act(exact)


def _ulp(t, dtype):
    """One unit in the last place of `dtype` at the magnitude of t (float64), the subnormal spacing below the normal range."""
    mant, emin = (10, -14) if dtype == F16 else (23, -126)
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def _views(x64, dtype, xoff, xpad, yoff, ypad):
    npix, C = x64.shape
    xb = torch.full((npix, xoff + C + xpad), NAN, dtype=dtype, device=DEV)
    xb[:, xoff:xoff + C] = x64.to(device=DEV, dtype=dtype)
    yb = torch.full((npix, yoff + C + ypad), NAN, dtype=dtype, device=DEV)
    return xb, yb


def _guards_ok(yb, yoff, C):
    return bool(torch.isnan(yb[:, :yoff]).all()) and bool(torch.isnan(yb[:, yoff + C:]).all())


def _same(got, want):
    """Equal values (+-0 are equal), NaN in the same places."""
    got, want = got.double().cpu(), want.double()
    return bool(torch.equal(torch.isnan(got), torch.isnan(want))) and bool(torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)))


def _int_data(name, npix, C):
    """Small integers, scales in +-{0.5, 1, 2}, (half-)integer shifts: s * x + b is exact in fp16, so fused = unfused = exact."""
    x = torch.floor(synth.uniform(53, name + ".x", (npix, C)) * 17).double() - 8
    s = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])[torch.clamp((synth.uniform(53, name + ".s", (C,)) * 6).long(), max=5)]
    b = (torch.floor(synth.uniform(53, name + ".b", (C,)) * 33) - 16) / 2
    return x, s.float(), b.float()


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("npix", [1, 7, 144])
@pytest.mark.parametrize("C", [8, 24, 2048])
def test_exact_and_random(hip_lib, C, npix, dtype):
    G = 8 if dtype == F16 else 4
    name = f"ssa.{C}.{npix}"
    xi, s, b = _int_data(name, npix, C)
    xr = synth.normal(53, name + ".xr", (npix, C)).to(dtype).double()
    sr = (synth.uniform(53, name + ".sr", (C,), 0.5, 1.5) * (1 - 2 * (torch.arange(C) % 3 == 1).float())).float()
    br = synth.normal(53, name + ".br", (C,)).float()
    for aname, act, k in ACTS:
        # integer data: bit for bit
        xb, yb = _views(xi, dtype, 2 * G, G, G, 3 * G)
        assert _call(hip_lib, xb, yb, dtype, npix, C, xb.shape[1], 2 * G, yb.shape[1], G, s.to(DEV), b.to(DEV), act) == 0
        torch.cuda.synchronize()
        want, _ = _ref(xi, s, b, k)
        assert torch.equal(want.to(dtype).double(), want), "the case itself is not exact"
        assert _same(yb[:, G:G + C], want) and _guards_ok(yb, G, C), f"{name} {dtype} {aname}: integer data"
        # random data: within one ulp of the output type
        xb, yb = _views(xr, dtype, 2 * G, G, G, 3 * G)
        assert _call(hip_lib, xb, yb, dtype, npix, C, xb.shape[1], 2 * G, yb.shape[1], G, sr.to(DEV), br.to(DEV), act) == 0
        torch.cuda.synchronize()
        _, exact = _ref(xr, sr, br, k)
        err = ((yb[:, G:G + C].double().cpu() - exact).abs() / _ulp(exact, dtype)).max().item()
        assert err <= 1.0 and _guards_ok(yb, G, C), f"{name} {dtype} {aname}: {err:.3f} ulp"


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
def test_non_finite_inputs_follow_act_mul(hip_lib, dtype):
    C, npix = 8, 4
    x = torch.tensor([[float("-inf"), float("inf"), NAN, -3.0, 0.0, 2.0, -0.0, 5.0]] * npix, dtype=torch.float64)
    s, b = torch.ones(C), torch.zeros(C)
    for aname, act, k in ACTS:
        xb, yb = _views(x, dtype, 8, 8, 8, 8)
        assert _call(hip_lib, xb, yb, dtype, npix, C, xb.shape[1], 8, yb.shape[1], 8, s.to(DEV), b.to(DEV), act) == 0
        torch.cuda.synchronize()
        neg_inf = 0.0 if aname == "relu" else float("-inf")
        want = torch.tensor([[neg_inf, float("inf"), NAN, -3.0 * k, 0.0, 2.0, 0.0, 5.0]] * npix, dtype=torch.float64)
        assert _same(yb[:, 8:16], want), f"{dtype} {aname}: {yb[0, 8:16].tolist()}"
        assert _same(yb[:, 8:16], _ref(x, s, b, k)[0]) and _guards_ok(yb, 8, C)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
def test_unaligned_view_goes_element_by_element(hip_lib, dtype):
    """C = 13 at channel offset 3 of a 21-channel buffer, output at offset 5 of 19: no 16-byte group lines up."""
    npix, C = 37, 13
    xi, s, b = _int_data("ssa.unaligned", npix, C)
    xb, yb = _views(xi, dtype, 3, 5, 5, 1)
    assert _call(hip_lib, xb, yb, dtype, npix, C, 21, 3, 19, 5, s.to(DEV), b.to(DEV), _lib.FT_ACT_RELU) == 0
    torch.cuda.synchronize()
    assert _same(yb[:, 5:5 + C], _ref(xi, s, b, 0.0)[0]) and _guards_ok(yb, 5, C)


def test_in_place_and_recorded(hip_lib):
    """x and y the same view, recorded through hip_ops.record_scale_shift_act as the model records it."""
    N, H, W, C = 2, 3, 4, 24
    xi, s, b = _int_data("ssa.inplace", N * H * W, C)
    buf = torch.full((N, H, W, 40), NAN, dtype=F16, device=DEV)
    buf[..., 8:8 + C] = xi.view(N, H, W, C).to(device=DEV, dtype=F16)
    v = ActView(buf, C, 8)
    prog = make_program()
    record_scale_shift_act(prog, v, v, s.to(DEV), b.to(DEV), "relu")
    assert [n for n, _ in prog.calls] == ["ft_scale_shift_act_nhwc_fwd"]
    run_program(prog)
    flat = buf.view(-1, 40)
    assert _same(flat[:, 8:8 + C], _ref(xi, s, b, 0.0)[0]) and _guards_ok(flat, 8, C)


def test_more_items_than_one_grid_pass(hip_lib):
    """C = 8 in fp16 is one group per pixel: 2048 x 256 + 77 pixels need a second pass of the grid-stride loop."""
    npix, C = MAX_BLOCKS * 256 + 77, 8
    x = (torch.arange(npix * C, dtype=torch.float64).view(npix, C) % 31) - 15
    s = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 1.0, 2.0])
    b = torch.tensor([0.5, -1.0, 3.0, 0.0, -2.5, 7.0, 1.0, -4.0])
    xb, yb = _views(x, F16, 8, 0, 8, 8)
    assert _call(hip_lib, xb, yb, F16, npix, C, 16, 8, 24, 8, s.to(DEV), b.to(DEV), _lib.FT_ACT_RELU) == 0
    torch.cuda.synchronize()
    assert _same(yb[:, 8:16], _ref(x, s, b, 0.0)[0]) and _guards_ok(yb, 8, C)


def test_error_codes(hip_lib):
    C, npix = 8, 4
    xb, yb = _views(torch.zeros((npix, C), dtype=torch.float64), F16, 8, 0, 8, 0)
    s, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ok = dict(x=xb, y=yb, dtype=F16, npix=npix, C=C, xcs=16, xoff=8, ycs=16, yoff=8, scale=s, shift=b, act=_lib.FT_ACT_RELU)
    assert _call(hip_lib, **ok) == _lib.FT_OK
    for bad in (dict(x=None), dict(y=None), dict(scale=None), dict(shift=None), dict(npix=0), dict(C=0), dict(xcs=15), dict(ycs=12), dict(xoff=-8),
                dict(yoff=-1), dict(act=3), dict(act=-1), dict(x=xb.data_ptr() + 1)):
        assert _call(hip_lib, **dict(ok, **bad)) == _lib.FT_ERR_INVALID_ARG, bad
    assert hip_lib.ft_scale_shift_act_nhwc_fwd(xb.data_ptr(), yb.data_ptr(), 7, ctypes.c_longlong(npix), C, 16, 8, 16, 8, s.data_ptr(), b.data_ptr(),
                                               _lib.FT_ACT_RELU, ctypes.c_float(0.0), current_stream_handle(DEV)) == _lib.FT_ERR_INVALID_ARG
    assert _call(hip_lib, **dict(ok, npix=1 << 40)) == _lib.FT_ERR_UNSUPPORTED      # refused before anything is launched
    torch.cuda.synchronize()
