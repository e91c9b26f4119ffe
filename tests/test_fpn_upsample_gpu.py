"""ft_upsample_bilinear_ac_fwd alone, through the C ABI: the case table of tests/fpn_ref.py in fp16 and fp32, with and without the
per-channel scale, against the float64 reference (upsample_ac_ref) and its derived bound (upsample_ac_bound, which already holds
the half fp16 ulp of the store); bit for bit where every weight is 0, 0.5 or 1; channel windows inside wider buffers; refusals.

Measured on an MI355X (worst error / bound over the random-data rows): fp32 0.60; fp16 0.999 — there the bound is the half fp16 ulp
of the store, which some element of a few thousand attains.  The fp32 bound is sensitive to the coordinate rule: with the product
src = r * o contracted into l1 = src - i0 (one fused multiply-add) the error is 2.1 x the bound."""
import ctypes

import pytest
import torch

import fpn_ref
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_F16, FT_F32, check

pytestmark = pytest.mark.gpu
SENTINEL = 99.0
GUARD = 8                                     # elements around the output: 16 or 32 bytes, so the 16-byte alignment is kept
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
SCALED = pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _group(dtype):
    return 8 if dtype == torch.float16 else 4


def _round_up(v, m):
    return (v + m - 1) // m * m


def _run(hip_lib, x, ho, wo, dtype, scale=None, x_cstride=None, x_coff=0, y_cstride=None, y_coff=0):
    """x: NCHW CPU tensor whose values `dtype` holds exactly.  Returns the written window as NCHW float64 on the CPU, after checking
    that every element outside it — channels in front of y_coff and from y_coff + C on, and the guards around the buffer — still
    holds the sentinel."""
    N, C, hi, wi = x.shape
    G = _group(dtype)
    x_cstride = _round_up(x_coff + C, G) if x_cstride is None else x_cstride
    y_cstride = _round_up(y_coff + C, G) if y_cstride is None else y_cstride
    xb = torch.full((N, hi, wi, x_cstride), SENTINEL, dtype=dtype)
    xb[..., x_coff:x_coff + C] = x.permute(0, 2, 3, 1).to(dtype)
    xb = xb.cuda()
    n_out = N * ho * wo * y_cstride
    buf = torch.full((n_out + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    yb = buf[GUARD:GUARD + n_out].view(N, ho, wo, y_cstride)
    assert xb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
    sc = scale.float().cuda().contiguous() if scale is not None else None
    check(hip_lib.ft_upsample_bilinear_ac_fwd(xb.data_ptr(), yb.data_ptr(), _lib.dtype_code(dtype), N, C, hi, wi, ho, wo, x_cstride, x_coff,
                                              y_cstride, y_coff, sc.data_ptr() if sc is not None else None, _stream()),
          "ft_upsample_bilinear_ac_fwd")
    torch.cuda.synchronize()
    out = buf.cpu()
    win = out[GUARD:GUARD + n_out].view(N, ho, wo, y_cstride)
    outside = torch.ones(y_cstride, dtype=torch.bool)
    outside[y_coff:y_coff + C] = False
    assert bool((out[:GUARD] == SENTINEL).all()) and bool((out[GUARD + n_out:] == SENTINEL).all()), "wrote outside the output buffer"
    assert bool((win[..., outside] == SENTINEL).all()), "wrote outside the channel window [y_coff, y_coff + C)"
    assert bool((xb.cpu()[..., :x_coff] == SENTINEL).all()), "wrote into the input"
    return win[..., y_coff:y_coff + C].permute(0, 3, 1, 2).double()


def _data(name, shape, dtype):
    return synth.normal(7, "fpn.up.gpu." + name, shape).to(dtype).float()        # values the dtype holds exactly


def _scale(name, C):
    return synth.uniform(7, "fpn.up.gpu.scale." + name, (C,), 0.5, 1.5) * (1 - 2 * (torch.arange(C) % 3 == 1).float())   # both signs


def _check_bound(hip_lib, name, x, ho, wo, dtype, scale, **window):
    want, mag = fpn_ref.upsample_ac_ref(x, ho, wo, scale)
    got = _run(hip_lib, x, ho, wo, dtype, scale, **window)
    bound = fpn_ref.upsample_ac_bound(want, mag, scale, fp16=dtype == torch.float16)
    ratio = ((got - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{name} {dtype} scale={scale is not None}: worst error / derived bound {ratio:.3f}, max abs error {(got - want).abs().max().item():.3e}")
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the derived bound"


@pytest.mark.parametrize("case", fpn_ref.UPSAMPLE_CASES, ids=lambda c: c[0])
@DTYPES
@SCALED
def test_random_data_within_derived_bound(hip_lib, case, dtype, scaled):
    name, N, C, hi, wi, ho, wo = case
    _check_bound(hip_lib, name, _data(name, (N, C, hi, wi), dtype), ho, wo, dtype, _scale(name, C) if scaled else None)


@DTYPES
@SCALED
def test_half_weights_bit_exact(hip_lib, dtype, scaled):
    """5x4 -> 9x7 (out = 2 in - 1): every weight is 0, 0.5 or 1.  With small-integer data and power-of-two scales every product and
    sum is exact in fp32 and the result fits fp16, so the kernel must return the float64 reference itself."""
    N, C, hi, wi, ho, wo = 2, 24, 5, 4, 9, 7
    x = (torch.arange(N * C * hi * wi).reshape(N, C, hi, wi) * 7 % 33 - 16).float()
    scale = torch.tensor([0.25, -2.0, 1.0, 0.5, -0.125, 4.0]).repeat(C // 6) if scaled else None
    want, _ = fpn_ref.upsample_ac_ref(x, ho, wo, scale)
    assert torch.equal(want.to(dtype).double(), want)            # the reference's values exist in the dtype
    got = _run(hip_lib, x, ho, wo, dtype, scale)
    assert torch.equal(got, want)


@DTYPES
def test_identity_bit_exact(hip_lib, dtype):
    """4x4 -> 4x4, N = 3: the ratio is 1, every l1 is 0, and the output is the input bit for bit; a scale of ones changes nothing."""
    x = _data("identity", (3, 40, 4, 4), dtype)
    for scale in (None, torch.ones(40)):
        got = _run(hip_lib, x, 4, 4, dtype, scale)
        assert torch.equal(got.to(dtype).view(torch.int16 if dtype == torch.float16 else torch.int32),
                           x.to(dtype).view(torch.int16 if dtype == torch.float16 else torch.int32))


@DTYPES
def test_ratio0_and_single_output(hip_lib, dtype):
    """1x1 -> 2x2 (ratio 0: every output is the one input pixel) and 3x5 -> 1x1 (ho = wo = 1: the output is pixel (0, 0))."""
    x = _data("ratio0", (2, 16, 1, 1), dtype)
    assert torch.equal(_run(hip_lib, x, 2, 2, dtype), x.double().expand(2, 16, 2, 2))
    x = _data("to_1x1", (2, 8, 3, 5), dtype)
    assert torch.equal(_run(hip_lib, x, 1, 1, dtype), x[:, :, :1, :1].double())


@DTYPES
@SCALED
def test_channel_windows(hip_lib, dtype, scaled):
    """x_cstride > C with a non-zero x_coff, and a non-zero y_coff inside a wider pre-filled output: _run checks that nothing
    outside [y_coff, y_coff + C) changed; the input's other channels hold the sentinel, so reading them would show in the result."""
    N, C, hi, wi, ho, wo = 2, 24, 5, 4, 9, 7
    x = _data("windows", (N, C, hi, wi), dtype)
    _check_bound(hip_lib, "windows", x, ho, wo, dtype, _scale("windows", C) if scaled else None, x_cstride=48, x_coff=16, y_cstride=64, y_coff=32)
    # C no multiple of the group, inside a wider output: the element-wise last group stops at C
    x = _data("windows13", (1, 13, 3, 4), dtype)
    _check_bound(hip_lib, "windows13", x, 5, 9, dtype, _scale("windows13", 13) if scaled else None, x_cstride=32, x_coff=8, y_cstride=32, y_coff=16)


def test_more_images_than_the_grid_covers(hip_lib):
    """No cap on N: the grid's y extent ends at 65535 images and a workgroup strides over the rest.  65535 + 70 images of
    2x2 -> 3x3 x 8 fp16 channels (4.7 M output elements) hold the same data, so every output image must equal the first, and the first
    the reference; the guard behind the last image stays.  (Element offsets are size_t products of the image index throughout.)"""
    N, C = 65535 + 70, 8
    x1 = _data("many", (1, C, 2, 2), torch.float16)
    scale = _scale("many", C)
    want, mag = fpn_ref.upsample_ac_ref(x1, 3, 3, scale)
    xb = x1.permute(0, 2, 3, 1).half().cuda().expand(N, 2, 2, C).contiguous()
    buf = torch.full((N * 9 * C + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    yb = buf[:N * 9 * C].view(N, 3, 3, C)
    sc = scale.float().cuda()
    check(hip_lib.ft_upsample_bilinear_ac_fwd(xb.data_ptr(), yb.data_ptr(), FT_F16, N, C, 2, 2, 3, 3, C, 0, C, 0, sc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    first = yb[0].cpu().permute(2, 0, 1).double().unsqueeze(0)
    assert bool(((first - want).abs() <= fpn_ref.upsample_ac_bound(want, mag, scale, fp16=True)).all())
    bits = yb.view(torch.int16).view(N, -1)
    assert bool((bits == bits[0]).all()), "an image differs from image 0"
    assert bool((buf[N * 9 * C:] == SENTINEL).all())


def test_refusals(hip_lib):
    x = torch.zeros(2 * 4 * 4 * 32, dtype=torch.float16, device="cuda")
    y = torch.full((2 * 8 * 8 * 32,), SENTINEL, dtype=torch.float16, device="cuda")
    sc = torch.ones(32, device="cuda")

    def call(xp=None, yp=None, dtype=FT_F16, N=2, C=16, hi=4, wi=4, ho=8, wo=8, xs=32, xo=0, ys=32, yo=0):
        return hip_lib.ft_upsample_bilinear_ac_fwd(x.data_ptr() if xp is None else xp, y.data_ptr() if yp is None else yp, dtype, N, C, hi, wi, ho, wo,
                                                   xs, xo, ys, yo, sc.data_ptr(), _stream())
    for kw in (dict(N=0), dict(C=0), dict(hi=0), dict(wi=-1), dict(ho=0), dict(wo=0), dict(dtype=7),
               dict(xo=-8), dict(yo=-8), dict(xs=8), dict(ys=8), dict(xo=24), dict(yo=24),           # window outside the pixel
               dict(xo=4), dict(yo=4), dict(xs=36), dict(ys=36),                                     # fp16: multiples of 8
               dict(dtype=FT_F32, xo=2), dict(dtype=FT_F32, ys=34),                                  # fp32: multiples of 4
               dict(xp=x.data_ptr() + 2), dict(yp=y.data_ptr() + 8)):                                # 16-byte aligned bases
        assert call(**kw) == FT_ERR_INVALID_ARG, kw
    assert hip_lib.ft_upsample_bilinear_ac_fwd(None, y.data_ptr(), FT_F16, 2, 16, 4, 4, 8, 8, 32, 0, 32, 0, None, _stream()) == FT_ERR_INVALID_ARG
    assert hip_lib.ft_upsample_bilinear_ac_fwd(x.data_ptr(), None, FT_F16, 2, 16, 4, 4, 8, 8, 32, 0, 32, 0, None, _stream()) == FT_ERR_INVALID_ARG
    assert call(hi=(1 << 24) + 1) == FT_ERR_UNSUPPORTED and call(wo=(1 << 24) + 1) == FT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                      # a refused call launches nothing
    assert call(dtype=FT_F32, N=1, C=8, xs=16, ys=16, hi=2, wi=2, ho=4, wo=4) == 0         # (the same buffers read as fp32: accepted)
