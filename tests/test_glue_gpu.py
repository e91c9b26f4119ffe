"""The small kernels between the convs, each launched alone through the C ABI on torch-allocated buffers and compared with the
high-precision references of tests/glue_ref.py: the fused warp / concat stages between the stacked FlowNets, the x4 upsamplers,
the 3x3/s2 max-pool (fallback form and the one fused into the stem) and the NCHW <-> NHWC packers.  Shapes are the smallest that
reach every path of each kernel (a last partial wave, pads that differ in and out, one row / one column, clamped source columns,
every dispatch threshold); two cases are large because only a large map makes a second grid-stride trip happen.

Tolerances of the concat stages (from the number formats and the project's bar for these operators, not from what the kernels give):
  fp32  1e-5 max-abs, the bar of the Resample2d / ChannelNorm tests at this input scale.  One exception, from the number format
        alone: the two |flow| channels of ft_flow_fusion_concat get max(1e-5, |want| * 2^-23).  sqrtf(x*x + y*y) in fp32 carries
        2^-24 per square and per sum under the root (halved by it) and 2^-24 behind it = 2^-23 of the value, and the fp32 OUTPUT
        resolves no better than 2^-24 of it: 3e-5 at the 250-px vectors of these flows, 64 at the planted (1e9, -1e9).
  fp16  per element |want| * 2^-10 + 1e-5: one fp16 ulp (half for the store's rounding, the rest for an fp32 result that lands on
        the other side of a rounding boundary).
Worst err / bound measured on an MI355X over all cases of a kernel (every case prints its own):
  ft_flow_warp_concat     fp32 0.076 (7.6e-7 on flow / div_flow = 24)      fp16 0.497
  ft_flow_fusion_concat   fp32 0.894 (|flow| = 262.7: 2.8e-5, one fp32 ulp; its 1e-5 channels: 0.037)      fp16 0.500
  ft_upsample_bilinear4x  0.030 (bound 1e-5 * max(1, |mul|))
Everything else in this module is exact (torch.equal)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import check
from glue_ref import BIG_SHAPE, CONCAT_SHAPES, DIV_FLOW

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
SENTINEL = 9.0


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bounds(want, dtype, loose_channels=()):
    """Per-element error bound for `want` [B,C,H,W] (float64): see the module docstring."""
    if dtype == torch.float16:
        return np.abs(want) * 2.0 ** -10 + 1e-5
    bound = np.full_like(want, 1e-5)
    for c in loose_channels:
        bound[:, c] = np.maximum(1e-5, np.abs(want[:, c]) * 2.0 ** -23)
    return bound


def _x6_buffer(x6, xl, xp, dtype):
    """NHWC [B,H,xp,8] on the GPU, the six image channels in columns [xl, xl + W), the sentinel everywhere else — in the pad
    columns too, so that a tap read from one shows."""
    B, _, H, W = x6.shape
    buf = torch.full((B, H, xp, 8), SENTINEL, dtype=dtype, device="cuda")
    buf[:, :, xl:xl + W, :6] = torch.from_numpy(x6).permute(0, 2, 3, 1).to("cuda", dtype)
    return buf


def _run_warp(hip_lib, x6, flow, shape, dtype):
    B, H, W, xl, xp, yl, yp = shape
    gx, gf = _x6_buffer(x6, xl, xp, dtype), torch.from_numpy(flow).cuda()
    y = torch.full((B, H, yp, 16), SENTINEL, dtype=dtype, device="cuda")
    check(hip_lib.ft_flow_warp_concat(gx.data_ptr(), gf.data_ptr(), ctypes.c_float(DIV_FLOW), y.data_ptr(), B, H, W, xl, xp, yl, yp,
                                      _lib.dtype_code(dtype), _stream()))
    torch.cuda.synchronize()
    return gx, y


def _run_fusion(hip_lib, x6, fsd, fs2, shape, dtype):
    B, H, W, xl, xp, yl, yp = shape
    gx, gsd, gs2 = _x6_buffer(x6, xl, xp, dtype), torch.from_numpy(fsd).cuda(), torch.from_numpy(fs2).cuda()
    y = torch.full((B, H, yp, 16), SENTINEL, dtype=dtype, device="cuda")
    check(hip_lib.ft_flow_fusion_concat(gx.data_ptr(), gsd.data_ptr(), gs2.data_ptr(), y.data_ptr(), B, H, W, xl, xp, yl, yp,
                                        _lib.dtype_code(dtype), _stream()))
    torch.cuda.synchronize()
    return gx, y


def _check_values(got_nhwc, want, dtype, what, loose_channels=()):
    """got_nhwc: [B,H,W,C] of the data columns; want: float64 [B,C,H,W].  Prints the worst err / bound, then asserts."""
    got = got_nhwc.permute(0, 3, 1, 2).double().cpu().numpy()
    err, bound = np.abs(got - want), _bounds(want, dtype, loose_channels)
    ratio = err / bound
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{what}: worst err / bound {ratio[worst]:.3f} (err {err[worst]:.3e}, want {want[worst]:.6g}, at {tuple(int(i) for i in worst)})")
    if loose_channels and dtype == torch.float32:
        strict = [c for c in range(want.shape[1]) if c not in loose_channels]
        print(f"{what}: worst err / bound of the 1e-5 channels {ratio[:, strict].max():.3f}")
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert ratio[worst] <= 1.0, f"{what}: err {err[worst]:.3e} > bound {bound[worst]:.3e} at {worst}"


# ---- ft_flow_warp_concat ------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shape", CONCAT_SHAPES, ids=str)
def test_flow_warp_concat(hip_lib, shape, dtype):
    """(img0, img1, warp(img1, flow), flow / div_flow, |img0 - warp|) vs the float64 reference: far out-of-frame vectors, zero and
    integer vectors, pads that differ in and out, the fp16 store path (lanes trade 16-byte pieces) and its fallback for a last
    partial wave, one row / one column; the call zeroes channels 12..15 and every pad column itself."""
    B, H, W, xl, xp, yl, yp = shape
    fp16 = dtype == torch.float16
    x6 = glue_ref.make_images(31, f"warp.x6.{shape}", B, H, W, fp16)
    flow = glue_ref.make_flow(31, f"warp.flow.{shape}", B, H, W, fp16)
    want = glue_ref.warp_concat_ref(x6, flow, DIV_FLOW)
    gx, y = _run_warp(hip_lib, x6, flow, shape, dtype)
    live = y[:, :, yl:yl + W]
    _check_values(live[..., :12], want, dtype, f"warp_concat {shape} {dtype}")
    assert torch.all(y[..., 12:] == 0), "channels 12..15 must be zero everywhere"
    assert torch.all(y[:, :, :yl] == 0) and torch.all(y[:, :, yl + W:] == 0), "the call zeroes the pad columns (all 16 channels)"
    assert torch.equal(live[..., :6], gx[:, :, xl:xl + W, :6]), "img0 | img1 pass through bit for bit"
    if B > 1:   # a batch-index slip would repeat one entry's result (each entry is also checked against its own reference above)
        assert not np.array_equal(want[0, 6:9], want[1, 6:9]) and not torch.equal(live[0, ..., 6:9], live[1, ..., 6:9])


# ---- ft_flow_fusion_concat ------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shape", CONCAT_SHAPES, ids=str)
def test_flow_fusion_concat(hip_lib, shape, dtype):
    """FlowNetFusion's 11-channel input from two independent flow fields vs the float64 reference, same shapes and flows as the
    warp stage; channels 11..15 of the data pixels are zero and — unlike ft_flow_warp_concat — the pad columns are left
    untouched, as the header says (the models zero that buffer once when they allocate it)."""
    B, H, W, xl, xp, yl, yp = shape
    fp16 = dtype == torch.float16
    x6 = glue_ref.make_images(32, f"fus.x6.{shape}", B, H, W, fp16)
    fsd = glue_ref.make_flow(32, f"fus.sd.{shape}", B, H, W, fp16)
    fs2 = glue_ref.make_flow(33, f"fus.s2.{shape}", B, H, W, fp16)
    want = glue_ref.fusion_concat_ref(x6, fsd, fs2)
    gx, y = _run_fusion(hip_lib, x6, fsd, fs2, shape, dtype)
    live = y[:, :, yl:yl + W]
    _check_values(live[..., :11], want, dtype, f"fusion_concat {shape} {dtype}", loose_channels=(7, 8))
    assert torch.all(live[..., 11:] == 0), "channels 11..15 of the data pixels must be zero"
    assert torch.all(y[:, :, :yl] == SENTINEL) and torch.all(y[:, :, yl + W:] == SENTINEL), "pad columns are not this call's to write"
    assert torch.equal(live[..., :3], gx[:, :, xl:xl + W, :3]), "img0 passes through bit for bit"
    if not fp16:
        assert torch.equal(live[..., 3:5].cpu(), torch.from_numpy(fsd).permute(0, 2, 3, 1)), "flow_sd passes through bit for bit"
        assert torch.equal(live[..., 5:7].cpu(), torch.from_numpy(fs2).permute(0, 2, 3, 1)), "flow_s2 passes through bit for bit"
    if B > 1:
        assert not torch.equal(live[0, ..., 9:11], live[1, ..., 9:11])


# ---- both, past the grid cap --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_inputs():
    """One image and two flow fields of BIG_SHAPE's map (every batch entry holds the same), the image rounded to fp16 and the
    flows within +-3000 so that the fp32 and the fp16 cases share them, and their float64 references: computed once."""
    _, H, W = BIG_SHAPE[:3]
    x6 = glue_ref.make_images(34, "big.x6", 1, H, W, fp16=True)
    fa = glue_ref.make_flow(34, "big.flow.a", 1, H, W, fp16=True)
    fb = glue_ref.make_flow(35, "big.flow.b", 1, H, W, fp16=True)
    want_warp = glue_ref.warp_concat_ref(x6, fa, DIV_FLOW)
    want_fusion = glue_ref.fusion_concat_ref(x6, fa, fb)
    for a in (x6, fa, fb, want_warp, want_fusion):
        a.setflags(write=False)
    return x6, fa, fb, want_warp, want_fusion


@DTYPES
@pytest.mark.parametrize("op", ["warp", "fusion"])
def test_concat_stages_past_the_grid_cap(hip_lib, op, dtype):
    """LARGE ON PURPOSE: both launches are capped at 16384 workgroups of 256 threads = 4 194 304 pixels per grid-stride trip, and
    the largest shape any other test runs (16 x 384 x 512) stays below that, so the loop's second trip was never executed.
    5 x 832 x 1024 (row pitch 1030) is the smallest round shape past the cap: 4 284 800 physical pixels for the warp stage,
    4 259 840 image pixels for the fusion stage; the second trip lands in the last batch entry.  All five entries hold the
    same image and flows: entry 0 is judged against the float64 reference (one image's worth, shared by all four cases),
    entries 1..4 must equal entry 0 bit for bit."""
    shape = BIG_SHAPE
    B, H, W, xl, xp, yl, yp = shape
    assert B * H * (yp if op == "warp" else W) > 16384 * 256
    x1, fa1, fb1, want_warp, want_fusion = _big_inputs()
    rep = lambda a: np.broadcast_to(a, (B,) + a.shape[1:]).copy()
    if op == "warp":
        _, y = _run_warp(hip_lib, rep(x1), rep(fa1), shape, dtype)
        want, nch, loose = want_warp, 12, ()
    else:
        _, y = _run_fusion(hip_lib, rep(x1), rep(fa1), rep(fb1), shape, dtype)
        want, nch, loose = want_fusion, 11, (7, 8)
    live = y[:, :, yl:yl + W]
    _check_values(live[:1, ..., :nch], want, dtype, f"{op}_concat past the grid cap {dtype}", loose_channels=loose)
    for b in range(1, B):
        assert torch.equal(y[b], y[0]), f"batch entry {b} differs from entry 0"
    assert torch.all(live[0, ..., nch:] == 0)
    pad_value = 0.0 if op == "warp" else SENTINEL
    assert torch.all(y[0, :, :yl] == pad_value) and torch.all(y[0, :, yl + W:] == pad_value)


# ---- x4 upsamplers ------------------------------------------------------------------------------------------------------------
UP_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 7), (2, 2, 5, 1), (1, 2, 2, 2), (3, 2, 33, 65)]


@pytest.mark.parametrize("mul", [20.0, -0.05])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=str)
def test_upsample_bilinear4x(hip_lib, shape, mul):
    """nn.Upsample(scale_factor=4, mode='bilinear') of x * mul vs torch in float64.  The kernel loads three source columns per
    cell and picks each tap among them BY VALUE of its clamped index, so the shapes that matter are those where the clamped
    columns coincide: one column, two columns, one row; plus a ragged multi-workgroup map."""
    N, C, h, w = shape
    x = synth.normal(41, f"bil{shape}", shape)
    gx = x.cuda()
    y = torch.full((N, C, 4 * h, 4 * w), SENTINEL, dtype=torch.float32, device="cuda")
    check(hip_lib.ft_upsample_bilinear4x(gx.data_ptr(), y.data_ptr(), N, C, h, w, ctypes.c_float(mul), _stream()))
    torch.cuda.synchronize()
    want = glue_ref.upsample_bilinear4x_ref(x, mul)
    err = (y.cpu().double() - want).abs().max().item()
    bound = 1e-5 * max(1.0, abs(mul))
    print(f"upsample_bilinear4x {shape} mul {mul}: worst err / bound {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("mul", [20.0, -0.05])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=str)
def test_upsample_nearest4x(hip_lib, shape, mul):
    """nn.Upsample(scale_factor=4, mode='nearest') of x * mul: one fp32 product, then copies — bit-equal to torch."""
    N, C, h, w = shape
    x = synth.normal(42, f"near{shape}", shape)
    gx = x.cuda()
    y = torch.full((N, C, 4 * h, 4 * w), SENTINEL, dtype=torch.float32, device="cuda")
    check(hip_lib.ft_upsample_nearest4x(gx.data_ptr(), y.data_ptr(), N, C, h, w, ctypes.c_float(mul), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), glue_ref.upsample_nearest4x_ref(x, mul))


# ---- 3x3 / stride 2 / pad 1 max-pool ----------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 8), (2, 7, 9, 24), (2, 8, 6, 8), (1, 2, 2, 16), (3, 33, 18, 64)]


def _pool(hip_lib, x, dtype):
    N, Hi, Wi, C = x.shape
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    gx = x.to("cuda", dtype)
    y = torch.full((N, Ho, Wo, C), SENTINEL, dtype=dtype, device="cuda")
    check(hip_lib.ft_maxpool3x3s2_fwd(gx.data_ptr(), y.data_ptr(), N, Hi, Wi, C, _lib.dtype_code(dtype), _stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _assert_same_with_nan(got, want, what):
    assert got.shape == want.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN positions differ ({int(torch.isnan(got).sum())} vs {int(torch.isnan(want).sum())})"
    keep = ~torch.isnan(want)
    assert torch.equal(got[keep], want[keep]), what


@DTYPES
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=str)
def test_maxpool_negative_inputs(hip_lib, shape, dtype):
    """nn.MaxPool2d(3, 2, 1) on strictly negative data: a padding value of 0 instead of -inf would win every border window (the
    stem + pool test only ever feeds this kernel post-ReLU data, where it could not).  A maximum is exact: torch.equal."""
    x = -synth.normal(51, f"pool{shape}", shape).abs() - 0.1
    x = x.to(dtype).float()                                     # the dtype-rounded values, for the kernel and for torch
    got = _pool(hip_lib, x, dtype)
    want = glue_ref.maxpool3x3s2_ref(x)
    assert bool((want < 0).all())
    assert torch.equal(got.float(), want)


@DTYPES
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=str)
def test_maxpool_non_finite_inputs(hip_lib, shape, dtype):
    """-inf, +inf and NaN among negative data, at border and at interior pixels: a window of nothing but -inf gives -inf, +inf
    wins, and a NaN anywhere in the window gives NaN as nn.MaxPool2d does (fmaxf, which the kernel used to take the maximum with,
    returns the other operand)."""
    N, Hi, Wi, C = shape
    x = -synth.normal(52, f"poolnf{shape}", shape).abs() - 0.1
    u = synth.uniform(52, f"poolnf.u{shape}", shape)
    x[u < 0.30] = float("-inf")                                 # enough of them for whole windows of -inf
    x[u > 0.97] = float("inf")
    x[(u > 0.60) & (u < 0.62)] = float("nan")
    # planted for certain: a NaN in a corner (border windows) and, where the map has one, at an interior pixel; +inf beside a NaN
    x[0, 0, 0, 0] = float("nan")
    x[-1, Hi - 1, Wi - 1, C - 1] = float("nan")
    if Hi > 2 and Wi > 2:
        x[0, Hi // 2, Wi // 2, 1] = float("nan")
        x[0, Hi // 2, Wi // 2 - 1, 1] = float("inf")
        x[-1, 1, 1, 2] = float("nan")
    x = x.to(dtype).float()
    got = _pool(hip_lib, x, dtype)
    want = glue_ref.maxpool3x3s2_ref(x)
    assert torch.isnan(want).any()
    _assert_same_with_nan(got.float(), want, f"maxpool {shape} {dtype}")


def test_fused_stem_pool_of_non_finite_values(hip_lib):
    """conv_stem_pool_kernel (the stem with its max-pool inside the launch, fp16): +NaN, -inf and +inf planted through the bias as
    in test_relu_of_non_finite_values must leave the pool as NaN, 0 and +inf, as relu + max_pool2d of torch; every other channel
    still matches the oracle.  (ReLU and the pool are integer maxima on the fp16 bit patterns there: a NaN whose SIGN bit is set
    orders below +0 and is dropped — DESIGN.md; not covered here.)"""
    from flowtrack.pytorch_amd.hip_ops import FusedConv, new_act, new_rowpacked_act, record_pack_input
    from util import make_program, run_program, view_to_nchw
    N, H, W = 2, 64, 48
    dev, dtype = torch.device("cuda:0"), torch.float16
    w = synth.normal(53, "sp.w", (64, 3, 7, 7), std=(2.0 / 147) ** 0.5).half().float()
    x = synth.normal(53, "sp.x", (N, 3, H, W)).half().float()
    bias = synth.normal(53, "sp.b", (64,), std=0.2)
    bias[1], bias[2], bias[3] = float("-inf"), float("inf"), float("nan")
    layer = FusedConv(w, stride=2, pad=3, bias=bias, act="relu", dtype=dtype, device=dev, label="stem_pool_nonfinite")
    fused_in = new_rowpacked_act(N, H, W, 3, 5, dtype, dev)
    pooled = new_act(N, H // 4, W // 4, 64, dtype, dev)
    pooled.t.fill_(SENTINEL)
    prog = make_program()
    record_pack_input(prog, x.to(dev), fused_in)
    layer.record(prog, fused_in, pooled, pool=True)
    run_program(prog)
    got = view_to_nchw(pooled)
    want = F.max_pool2d(F.relu(F.conv2d(x, w, bias, stride=2, padding=3)), 3, 2, 1)
    assert torch.all(got[:, 1] == 0.0), "pool(ReLU(-inf)) must be 0"
    assert torch.all(torch.isposinf(got[:, 2])), "pool(ReLU(+inf)) must stay +inf"
    assert torch.all(torch.isnan(got[:, 3])), "pool(ReLU(NaN)) must stay NaN"
    assert torch.all(want[:, 1] == 0.0) and torch.all(torch.isposinf(want[:, 2])) and torch.all(torch.isnan(want[:, 3]))
    keep = [c for c in range(64) if c not in (1, 2, 3)]
    scale = max(1.0, want[:, keep].abs().max().item())
    assert (got[:, keep] - want[:, keep]).abs().max().item() <= 2e-2 * scale


# ---- NHWC -> NCHW -------------------------------------------------------------------------------------------------------------
UNPACK_CASES = [(2, 3, 5, 7, 8, 0), (1, 17, 4, 6, 32, 8), (3, 2, 9, 11, 16, 13), (1, 441, 3, 5, 480, 32)]


@DTYPES
@pytest.mark.parametrize("case", UNPACK_CASES, ids=str)
def test_unpack_nhwc_to_nchw(hip_lib, case, dtype):
    """A channel slice (stride / offset) of an NHWC buffer -> NCHW fp32, bit-equal to the permuted slice; one guard element on
    each side of the output stays untouched."""
    N, C, H, W, cs, coff = case
    x = synth.normal(61, f"unpack{case}", (N, H, W, cs)).to(dtype)
    gx = x.cuda()
    n = N * C * H * W
    buf = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device="cuda")
    check(hip_lib.ft_unpack_nhwc_to_nchw(gx.data_ptr(), buf.data_ptr() + 4, N, C, H, W, cs, coff, _lib.dtype_code(dtype), _stream()))
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[1:-1].view(N, C, H, W), glue_ref.unpack_ref(x, C, coff))
    assert got[0] == SENTINEL and got[-1] == SENTINEL, "wrote outside its output"


def test_unpack_refuses_invalid_arguments(hip_lib):
    x = torch.zeros((1, 2, 2, 8), dtype=torch.float32, device="cuda")
    y = torch.full((32,), SENTINEL, dtype=torch.float32, device="cuda")
    call = lambda xp, yp, C, cs, coff, code=_lib.FT_F32: hip_lib.ft_unpack_nhwc_to_nchw(xp, yp, 1, C, 2, 2, cs, coff, code, _stream())
    assert call(x.data_ptr(), y.data_ptr(), 4, 8, 5) != 0          # x_cstride < x_coff + C
    assert call(x.data_ptr(), y.data_ptr(), 4, 8, -1) != 0         # negative offset
    assert call(None, y.data_ptr(), 4, 8, 0) != 0                  # null pointers
    assert call(x.data_ptr(), None, 4, 8, 0) != 0
    assert call(x.data_ptr(), y.data_ptr(), 4, 8, 0, 7) != 0       # unknown dtype
    assert call(x.data_ptr(), y.data_ptr(), 4, 8, 4) == 0          # the slice that just fits
    torch.cuda.synchronize()
    assert torch.all(y[16:] == SENTINEL) and torch.all(y[:16] == 0)


# ---- NCHW -> NHWC -------------------------------------------------------------------------------------------------------------
PACK_CASES = [
    # dtype, C, cpad, W, byte offset of x from its 16-byte boundary
    (torch.float32, 3, 4, 12, 0), (torch.float32, 5, 8, 12, 0), (torch.float32, 3, 4, 7, 0), (torch.float32, 5, 8, 7, 0),
    (torch.float16, 5, 8, 12, 0), (torch.float16, 5, 8, 7, 0),
    (torch.float16, 3, 4, 12, 4),     # W % 4 == 0 and C <= 3, but x not 16-byte aligned: the generic kernel, not the 4-pixel one
    (torch.float16, 3, 4, 12, 0),     # the same on the 4-pixel kernel
]


@pytest.mark.parametrize("rowpacked", [False, True], ids=["plain", "lpad3"])
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"{str(c[0])[6:]}-C{c[1]}-cpad{c[2]}-W{c[3]}-off{c[4]}")
def test_pack_nchw_to_nhwc(hip_lib, case, rowpacked):
    """NCHW fp32 -> NHWC fp16 / fp32 with channel padding 4 and 8, plain and row-packed: data in columns [lpad, lpad + W), every
    padding channel and column exactly zero although the buffer held garbage."""
    dtype, C, cpad, W, off = case
    N, H = 2, 5
    lpad, wpitch = (3, W + 6) if rowpacked else (0, W)
    x = synth.normal(62, f"pack{C}{W}", (N, C, H, W))
    flat = torch.full((x.numel() + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0 and off % 4 == 0
    flat[off // 4:off // 4 + x.numel()] = x.flatten().cuda()
    y = torch.full((N, H, wpitch, cpad), SENTINEL, dtype=dtype, device="cuda")
    check(hip_lib.ft_pack_nchw_to_nhwc(flat.data_ptr() + off, y.data_ptr(), N, C, H, W, cpad, lpad, wpitch, _lib.dtype_code(dtype), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), glue_ref.pack_ref(x, cpad, lpad, wpitch, dtype))
