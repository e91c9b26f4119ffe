"""The one-launch top-down step of the lateral-deconv pose head, the kernel alone through the C ABI: ft_conv2d_fwd with the K-concat second
input (ft_conv_desc.x2_*) behind transposed = 1,

    y[n, oy, ox, :] = act(scale .* (ConvT(x)[n, oy, ox, :] + W2 . x2[n, oy, ox, :]) + shift).

The weights are packed by the numpy restatement of the layout (tests/posenet_ref.py::pack_taps_w2) with the geometry the library reports,
so the host packer (hip_ops.FusedLateralDeconv) is a separate subject with a test of its own here.  References are float64:
  * random data under the derived bound of tests/conv_bound.py with K = 4 Cin + x2_cin (fp32: the same accumulation term, 2^-24 |want|
    for the fused multiply-add of the epilogue in place of the fp16 rounding — fp32 products are not exact, one more 2^-24 S);
  * integer data (integer inputs, +-1 weights, power-of-two scales: tests/exact_cases.py) element for element;
  * impulses: a one-hot in x2 must give W2's column at that output pixel and zeros elsewhere (a wrong phase offset moves it), a one-hot
    in x must give the bits of the same descriptor without x2.
Every case runs hint 0 and every hint of ft_conv_tile_candidates; x, x2 and y are channel slices of wider buffers whose other channels
hold NaN (the padding of a K-run inside the slice is zero, as in every activation buffer: the kernel reads it against zero weights).
Also here: the deconv of the two-launch form, transposed + residual + scale without a shift, which no other test holds."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as ec
import posenet_ref
from conv_bound import derived_bound
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import ConvDesc, ConvGeometry
from flowtrack.pytorch_amd.hip_ops import (WIDE8, ActView, FusedConv, FusedLateralDeconv, act_stride, current_stream_handle, decode_tile, round_up,
                                           tile_str)
from util import make_program, run_program, view_to_nchw

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
NAN = float("nan")
ACTS = {None: _lib.FT_ACT_NONE, "relu": _lib.FT_ACT_RELU, "leaky": _lib.FT_ACT_LEAKY}


def _bk(dtype):
    return 32 if dtype == F16 else 16          # channels of one K-step


def _slice_view(x64, dtype, coff, run_pad):
    """x64 [N,C,H,W] as channels [coff, coff + C) of a buffer [NaN x coff | C data | zeros up to run_pad | NaN x 32]."""
    N, C, H, W = x64.shape
    buf = torch.full((N, H, W, coff + run_pad + 32), NAN, dtype=dtype, device=DEV)
    buf[..., coff:coff + run_pad] = 0
    buf[..., coff:coff + C] = x64.permute(0, 2, 3, 1).to(device=DEV, dtype=dtype)
    return ActView(buf, C, coff)


def _out_view(N, H, W, C, dtype, coff=8):
    return ActView(torch.full((N, H, W, coff + round_up(C, 8) + 8), NAN, dtype=dtype, device=DEV), C, coff)


def _desc(dtype, xv, yv, cout, x2v=None, act=None, slope=0.0):
    d = ConvDesc()
    d.dtype = _lib.dtype_code(dtype)
    d.N, d.Hi, d.Wi = xv.N, xv.H, xv.W
    d.Cin, d.x_cstride, d.x_coff = xv.C, xv.cstride, xv.coff
    d.Cout, d.kh, d.kw, d.stride, d.pad, d.transposed = cout, 4, 4, 2, 1, 1
    d.Ho, d.Wo = 2 * xv.H, 2 * xv.W
    d.y_cstride, d.y_coff, d.out_layout = yv.cstride, yv.coff, _lib.FT_LAYOUT_NHWC
    d.act, d.slope = ACTS[act], slope
    if x2v is not None:
        d.x2_cin, d.x2_hi, d.x2_wi, d.x2_cstride, d.x2_coff, d.x2_stride = x2v.C, x2v.H, x2v.W, x2v.cstride, x2v.coff, 1
    return d


def _geometry(lib, d):
    g = ConvGeometry()
    assert lib.ft_conv_pack_geometry(ctypes.byref(d), ctypes.byref(g)) == 0
    return g


def _hints(lib, d):
    hints = (ctypes.c_int * 64)()
    n = lib.ft_conv_tile_candidates(ctypes.byref(d), hints, 64)
    assert n >= 0
    return [int(v) for v in hints[:n]]


def _hint_str(h):
    return f"hint {h:#x} ({tile_str(h)})"


def _table(v, cout_pad):
    if v is None:
        return None
    t = torch.zeros(cout_pad, dtype=torch.float32)
    t[:v.numel()] = v.float()
    return t.to(DEV)


class Step:
    """One launch set up through the C ABI: views, the packed [taps | W2] matrix, scale / shift tables."""

    def __init__(self, lib, dtype, x64, x2_64, wt64, w2_64, scale=None, shift=None, act=None, slope=0.0, xoff=32, x2off=32):
        self.lib, self.dtype = lib, dtype
        N, cin, hi, wi = x64.shape
        cout = wt64.shape[1]
        bk = _bk(dtype)
        self.xv = _slice_view(x64, dtype, xoff, round_up(cin, bk))
        self.x2v = _slice_view(x2_64, dtype, x2off, round_up(x2_64.shape[1], bk)) if x2_64 is not None else None
        self.yv = _out_view(N, 2 * hi, 2 * wi, cout, dtype)
        self.d = _desc(dtype, self.xv, self.yv, cout, self.x2v, act, slope)
        g = self.g = _geometry(lib, self.d)
        assert (g.nphases, g.ntaps, g.cin_pad, g.cin2_pad) == (4, 4, round_up(cin, bk), round_up(x2_64.shape[1], bk) if x2_64 is not None else 0)
        assert g.kpad == 4 * g.cin_pad + g.cin2_pad
        if x2_64 is not None:
            packed = posenet_ref.pack_taps_w2(wt64.numpy(), w2_64.numpy(), g.cin_pad, g.cin2_pad, g.cout_pad)
        else:
            packed = posenet_ref.pack_taps_w2(wt64.numpy(), np.zeros((cout, 0, 1, 1)), g.cin_pad, 0, g.cout_pad)
        self.w = torch.from_numpy(packed).to(device=DEV, dtype=dtype).contiguous()
        self.scale, self.shift = _table(scale, g.cout_pad), _table(shift, g.cout_pad)

    def run(self, hint=0):
        self.d.tile_hint = hint
        self.yv.t.fill_(NAN)
        rc = self.lib.ft_conv2d_fwd(ctypes.byref(self.d), self.xv.t.data_ptr(), self.w.data_ptr(),
                                    self.scale.data_ptr() if self.scale is not None else None,
                                    self.shift.data_ptr() if self.shift is not None else None,
                                    self.x2v.t.data_ptr() if self.x2v is not None else None, self.yv.t.data_ptr(), current_stream_handle(DEV))
        assert rc == 0, f"ft_conv2d_fwd returned {rc} ({_hint_str(hint)})"
        torch.cuda.synchronize()
        y = self.yv
        assert bool(torch.isnan(y.t[..., :y.coff]).all()) and bool(torch.isnan(y.t[..., y.coff + y.C:]).all()), "channels outside the output slice were written"
        return view_to_nchw(y).double()

    def hints(self):
        hs = _hints(self.lib, self.d)
        for h in hs:      # what the header states: with a second input no split-K, halo or 8-phase form is offered
            t = decode_tile(h)
            assert t.sk == 1 and t.ks == 1 and not t.halo and t.wide != WIDE8, _hint_str(h)
        assert self.lib.ft_conv_workspace_bytes(ctypes.byref(self.d)) == 0
        return hs


def _ref(x, x2, wt, w2, scale, shift, act, slope=0.0):
    """(want, pre, S) in float64: pre = the unscaled sum, S = the sum of the magnitudes of its products."""
    pre = F.conv_transpose2d(x, wt, stride=2, padding=1)
    S = F.conv_transpose2d(x.abs(), wt.abs(), stride=2, padding=1)
    if x2 is not None:
        pre = pre + F.conv2d(x2, w2)
        S = S + F.conv2d(x2.abs(), w2.abs())
    v = pre
    if scale is not None:
        v = v * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        v = v + shift.double().view(1, -1, 1, 1)
    if act == "relu":
        v = v.clamp(min=0)
    elif act == "leaky":
        v = torch.where(v > 0, v, v * slope)
    return v, pre, S


def _bound(dtype, K, S, pre, scale, want):
    if dtype == F16:
        return derived_bound(K, S, pre, scale, want)
    # fp32: the accumulation term of derived_bound plus one 2^-24 S for the products (fp32 x fp32 is not exact), and one rounding of
    # the epilogue's multiply-add in place of the rounding to fp16
    return 2.0 * ((K + 1) * 2.0 ** -24 * S + 2.0 ** -23 * pre.abs()) * scale.abs().view(1, -1, 1, 1) + 2.0 ** -23 * want.abs() + 2.0 ** -126


def _rand(name, shape, dtype, mul=1.0):
    """float64 values the dtype holds exactly."""
    return (synth.normal(31, "dl." + name, shape) * mul).to(dtype).double()


def _rand_case(name, dtype, N, hi, wi, cin, cin2, cout, wmul=0.05):
    x = _rand(name + ".x", (N, cin, hi, wi), dtype)
    x2 = _rand(name + ".x2", (N, cin2, 2 * hi, 2 * wi), dtype)
    wt = _rand(name + ".wt", (cin, cout, 4, 4), dtype, wmul)
    w2 = _rand(name + ".w2", (cout, cin2, 1, 1), dtype, wmul)
    scale = (synth.uniform(31, "dl." + name + ".s", (cout,), 0.5, 1.5) * (1 - 2 * (torch.arange(cout) % 3 == 1).float())).float()   # both signs
    shift = synth.normal(31, "dl." + name + ".b", (cout,)).float()
    return x, x2, wt, w2, scale, shift


def _check_bound(step, x, x2, wt, w2, scale, shift, act, what, K):
    want, pre, S = _ref(x, x2, wt, w2, scale, shift, act)
    bound = _bound(step.dtype, K, S, pre, scale.double(), want)
    hints = step.hints()
    assert len(hints) >= 2, f"{what}: only {len(hints)} tile variants offered"
    worst = 0.0
    for h in [0] + hints:
        got = step.run(h)
        ratio = ((got - want).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what} {_hint_str(h)}: error / derived bound {ratio:.3f}"
    print(f"{what}: {len(hints)} hints, worst error / derived bound {worst:.3f}")


SMALL_SHAPES = [(1, 1, 1), (1, 2, 3), (3, 3, 5)]          # N, Hi, Wi: one pixel per phase; 2 x 3; a pixel count that is no multiple of any tile


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cout", [48, 256])
@pytest.mark.parametrize("cin2", [32, 40])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=["n1_1x1", "n1_2x3", "n3_3x5"])
def test_small_shapes_derived_bound(hip_lib, shape, cin2, cout, dtype):
    """The least channel counts the K-concat form accepts (two K-steps per tap: 64 fp16 / 32 fp32 channels), x2_cin = 32 and 40 (padding
    inside the K-run), Cout = 48 (a ragged 64-channel tile) and 256, random data, ReLU behind a BatchNorm of both signs."""
    N, hi, wi = shape
    cin = 64 if dtype == F16 else 32
    name = f"small.{N}.{hi}x{wi}.{cin2}.{cout}"
    x, x2, wt, w2, scale, shift = _rand_case(name, dtype, N, hi, wi, cin, cin2, cout)
    step = Step(hip_lib, dtype, x, x2, wt, w2, scale, shift, "relu")
    _check_bound(step, x, x2, wt, w2, scale, shift, "relu", f"{name} {dtype}", 4 * cin + cin2)


MODEL_ROWS = [(2, 2, 2048, 1024), (4, 3, 256, 512), (8, 6, 256, 256)]         # Hi, Wi, Cin, x2_cin of the head's three steps at N = 1


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("row", MODEL_ROWS, ids=["deconv1", "deconv2", "deconv3"])
def test_model_rows_derived_bound(hip_lib, row, dtype):
    hi, wi, cin, cin2 = row
    name = f"row.{hi}x{wi}.{cin}.{cin2}"
    x, x2, wt, w2, scale, shift = _rand_case(name, dtype, 1, hi, wi, cin, cin2, 256, wmul=0.02)
    step = Step(hip_lib, dtype, x, x2, wt, w2, scale, shift, "relu", xoff=0, x2off=0)
    _check_bound(step, x, x2, wt, w2, scale, shift, "relu", f"{name} {dtype}", 4 * cin + cin2)


def _int_case(name, N, hi, wi, cin, cin2, cout):
    """Integer inputs, +-1 weights (about 32 non-zero per row and run), power-of-two scales, (half-)integer shifts."""
    x = ec.int_input("dl." + name + ".x", (N, cin, hi, wi))
    x2 = ec.int_input("dl." + name + ".x2", (N, cin2, 2 * hi, 2 * wi))
    wt = ec.int_weights("dl." + name + ".wt", (cin, cout, 4, 4), 8.0 / cin, out_dim=1)
    w2 = ec.int_weights("dl." + name + ".w2", (cout, cin2, 1, 1), 32.0 / cin2)
    bn = ec.pow2_bn("dl." + name + ".bn", cout)
    scale, shift = ec.fold64(cout, None, bn)
    return x, x2, wt, w2, scale, shift


INT_CASES = [(N, hi, wi, None, cin2, cout) for (N, hi, wi) in SMALL_SHAPES for cin2, cout in ((32, 48), (40, 256))] + \
            [(1, hi, wi, cin, cin2, 256) for hi, wi, cin, cin2 in MODEL_ROWS]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", INT_CASES, ids=["n%d_%dx%d_cin%s_x2%d_cout%d" % c for c in INT_CASES])
def test_integer_data_is_exact(hip_lib, case, dtype):
    """Every product and every partial sum is exact and every stored value representable: element for element, every hint."""
    N, hi, wi, cin, cin2, cout = case
    cin = cin or (64 if dtype == F16 else 32)
    name = f"int.{N}.{hi}x{wi}.{cin}.{cin2}.{cout}"
    x, x2, wt, w2, scale, shift = _int_case(name, N, hi, wi, cin, cin2, cout)
    want, pre, _ = _ref(x, x2, wt, w2, scale, shift, "relu")
    assert torch.equal(want.half().double(), want) and pre.abs().max().item() < 2048, "the case itself is not exact in fp16"
    assert (want > 0).double().mean().item() > 0.1
    step = Step(hip_lib, dtype, x, x2, wt, w2, scale.float(), shift.float(), "relu")
    for h in [0] + step.hints():
        ec.assert_exact(step.run(h), want, f"{name} {dtype} {_hint_str(h)}")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
def test_x2_impulse_lands_on_its_pixel(hip_lib, dtype):
    """x = 0 and a one-hot in x2 at one output pixel: W2's column of that channel at that pixel, zero everywhere else, bit for bit.  The
    four image corners are the four output parities (Ho, Wo even); two interior pixels of mixed parity and the second image too."""
    N, hi, wi, cin2, cout = 2, 2, 3, 40, 48
    cin = 64 if dtype == F16 else 32
    ho, wo = 2 * hi, 2 * wi
    wt = _rand("imp.wt", (cin, cout, 4, 4), dtype, 0.05)
    w2 = _rand("imp.w2", (cout, cin2, 1, 1), dtype)
    x = torch.zeros((N, cin, hi, wi), dtype=torch.float64)
    pixels = [(0, 0, 0, 0), (0, 0, wo - 1, 7), (0, ho - 1, 0, 39), (0, ho - 1, wo - 1, 13), (1, 1, 2, 22), (1, 2, 3, 31)]      # n, oy, ox, channel
    assert {(oy & 1, ox & 1) for _, oy, ox, _ in pixels[:4]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for n, oy, ox, c in pixels:
        x2 = torch.zeros((N, cin2, ho, wo), dtype=torch.float64)
        x2[n, c, oy, ox] = 1.0
        step = Step(hip_lib, dtype, x, x2, wt, w2)
        want = torch.zeros((N, cout, ho, wo), dtype=torch.float64)
        want[n, :, oy, ox] = w2[:, c, 0, 0]
        for h in [0] + step.hints():
            ec.assert_exact(step.run(h), want, f"x2 one-hot at image {n} pixel ({oy}, {ox}) channel {c} {dtype} {_hint_str(h)}")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
def test_x_impulse_equals_plain_deconv(hip_lib, dtype):
    """x2 = 0 and a one-hot in x: the bits of the same descriptor without x2 (whose own parity is held by the existing suites)."""
    N, hi, wi, cin2, cout = 2, 2, 3, 40, 48
    cin = 64 if dtype == F16 else 32
    x, x2r, wt, w2, scale, shift = _rand_case("ximp", dtype, N, hi, wi, cin, cin2, cout)
    x2 = torch.zeros_like(x2r)
    for n, iy, ix, c in ((0, 0, 0, 0), (1, hi - 1, wi - 1, cin - 1), (0, 1, 1, 17)):
        x1 = torch.zeros_like(x)
        x1[n, c, iy, ix] = x[n, c, iy, ix] if x[n, c, iy, ix] != 0 else 1.0
        plain = Step(hip_lib, dtype, x1, None, wt, None, scale, shift, "relu").run(0)
        step = Step(hip_lib, dtype, x1, x2, wt, w2, scale, shift, "relu")
        for h in [0] + step.hints():
            got = step.run(h)
            assert torch.equal(got.float().view(torch.int32), plain.float().view(torch.int32)), f"x one-hot at ({n}, {iy}, {ix}, {c}) {dtype} {_hint_str(h)}"


def test_descriptor_refusals(hip_lib):
    """x2 not at the output geometry is an invalid argument; x2 together with a residual or a fused tail is unsupported; below two
    K-steps per tap the form is unsupported."""
    x = torch.zeros((1, 64, 2, 3), dtype=torch.float64)
    x2 = torch.zeros((1, 32, 4, 6), dtype=torch.float64)
    wt, w2 = torch.zeros((64, 64, 4, 4), dtype=torch.float64), torch.zeros((64, 32, 1, 1), dtype=torch.float64)
    step = Step(hip_lib, F16, x, x2, wt, w2)
    g = ConvGeometry()

    def status(**kw):
        d = ConvDesc.from_buffer_copy(step.d)
        for k, v in kw.items():
            setattr(d, k, v)
        rc = hip_lib.ft_conv_pack_geometry(ctypes.byref(d), ctypes.byref(g))
        rc2 = hip_lib.ft_conv2d_fwd(ctypes.byref(d), step.xv.t.data_ptr(), step.w.data_ptr(), None, None, step.x2v.t.data_ptr(), step.yv.t.data_ptr(),
                                    current_stream_handle(DEV))
        assert rc == rc2
        return rc
    assert status() == _lib.FT_OK
    assert status(x2_hi=2, x2_wi=3) == _lib.FT_ERR_INVALID_ARG                   # the INPUT geometry
    assert status(x2_stride=2) == _lib.FT_ERR_INVALID_ARG
    assert status(x2_hi=7, x2_wi=11, x2_stride=2) == _lib.FT_ERR_INVALID_ARG    # (the 1x1 form's rule would accept it: Ho = (7 - 1) / 2 + 1)
    assert status(x2_hi=5) == _lib.FT_ERR_INVALID_ARG and status(x2_wi=8) == _lib.FT_ERR_INVALID_ARG
    assert status(has_residual=1, res_cstride=64, res_coff=0) == _lib.FT_ERR_UNSUPPORTED
    assert status(tail_cout=17) == _lib.FT_ERR_UNSUPPORTED
    assert status(Cin=32) == _lib.FT_ERR_UNSUPPORTED                              # one K-step per tap
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
def test_host_packer_matches_the_restated_layout(hip_lib, dtype):
    """hip_ops.FusedLateralDeconv: its packed matrix equals pack_taps_w2's, its scale / shift are the BatchNorm's fold (not folded into
    the weights), it records ONE ft_conv2d_fwd, and the launch gives the integer case's exact result."""
    N, hi, wi, cin2, cout = 3, 3, 5, 40, 48
    cin = 64 if dtype == F16 else 32
    name = f"packer.{dtype}"
    x = ec.int_input("dl." + name + ".x", (N, cin, hi, wi))
    x2 = ec.int_input("dl." + name + ".x2", (N, cin2, 2 * hi, 2 * wi))
    wt = ec.int_weights("dl." + name + ".wt", (cin, cout, 4, 4), 8.0 / cin, out_dim=1)
    w2 = ec.int_weights("dl." + name + ".w2", (cout, cin2, 1, 1), 32.0 / cin2)
    bn = ec.pow2_bn("dl." + name + ".bn", cout)
    scale, shift = ec.fold64(cout, None, bn)
    want, _, _ = _ref(x, x2, wt, w2, scale, shift, "relu")
    bk = _bk(dtype)
    xv = _slice_view(x, dtype, 32, round_up(cin, bk))
    x2v = _slice_view(x2, dtype, 32, round_up(cin2, bk))
    yv = _out_view(N, 2 * hi, 2 * wi, cout, dtype)
    layer = FusedLateralDeconv(wt.float(), w2.float(), bn, dtype=dtype, device=DEV, act="relu", label=name)
    assert layer.supported(xv, x2v, yv)
    prog = make_program()
    layer.record(prog, xv, x2v, yv)
    assert [n for n, _ in prog.calls] == ["ft_conv2d_fwd"]
    d = prog.conv_records[0][3]
    assert d.transposed == 1 and d.x2_cin == cin2 and (d.x2_hi, d.x2_wi, d.x2_stride) == (2 * hi, 2 * wi, 1)
    g = _geometry(hip_lib, d)
    w, sc, sh = layer._packed_for(d)
    restated = posenet_ref.pack_taps_w2(wt.numpy(), w2.numpy(), g.cin_pad, g.cin2_pad, g.cout_pad)
    assert torch.equal(w.double().cpu(), torch.from_numpy(restated))
    assert torch.equal(sc[:cout].double().cpu(), scale) and torch.equal(sh[:cout].double().cpu(), shift)
    run_program(prog)
    ec.assert_exact(view_to_nchw(yv), want, name)
    assert bool(torch.isnan(yv.t[..., :yv.coff]).all()) and bool(torch.isnan(yv.t[..., yv.coff + yv.C:]).all())


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("row", MODEL_ROWS, ids=["deconv1", "deconv2", "deconv3"])
def test_two_launch_forms_deconv(hip_lib, row, dtype):
    """The "lateral+deconv" form's second launch as the model records it: a transposed conv with the BatchNorm's scale, NO shift, the
    lateral map as its residual input and ReLU — relu(s ConvT(x) + l) under the derived bound with K = 4 Cin and the residual add as
    one more fp32 operation."""
    hi, wi, cin, _ = row
    cout = 256
    name = f"two.{hi}x{wi}.{cin}"
    x = _rand(name + ".x", (1, cin, hi, wi), dtype)
    wt = _rand(name + ".wt", (cin, cout, 4, 4), dtype, 0.02)
    l = _rand(name + ".l", (1, cout, 2 * hi, 2 * wi), dtype)
    gamma = (synth.uniform(31, "dl." + name + ".s", (cout,), 0.5, 1.5) * (1 - 2 * (torch.arange(cout) % 3 == 1).float())).float()
    bn = {"weight": gamma, "bias": torch.zeros(cout), "running_mean": torch.zeros(cout), "running_var": torch.ones(cout), "eps": 0.0}
    layer = FusedConv(wt.float(), dtype=dtype, device=DEV, transposed=True, stride=2, pad=1, bn=bn, act="relu", label=name)
    xv = _slice_view(x, dtype, 0, act_stride(cin))
    lv = _slice_view(l, dtype, 0, act_stride(cout))
    yv = _out_view(1, 2 * hi, 2 * wi, cout, dtype)
    prog = make_program()
    layer.record(prog, xv, yv, residual=lv)
    prog.resolve_choices()
    assert len(prog.calls) == 1 and prog.conv_records[0][3].has_residual == 1
    run_program(prog)
    got = view_to_nchw(yv).double()
    pre = F.conv_transpose2d(x, wt, stride=2, padding=1)
    S = F.conv_transpose2d(x.abs(), wt.abs(), stride=2, padding=1)
    scale = gamma.double()
    want = (pre * scale.view(1, -1, 1, 1) + l).clamp(min=0)
    K = 4 * cin
    if dtype == F16:
        bound = derived_bound(K, S, pre, scale, want, extra=(pre * scale.view(1, -1, 1, 1) + l,))
    else:
        bound = _bound(dtype, K, S, pre, scale, want) + 2.0 ** -24 * (pre * scale.view(1, -1, 1, 1) + l).abs()
    ratio = ((got - want).abs() / bound).max().item()
    print(f"{name} {dtype} ({prog.calls[0][0]}): error / derived bound {ratio:.3f}")
    assert ratio <= 1.0
    assert bool(torch.isnan(yv.t[..., :yv.coff]).all()) and bool(torch.isnan(yv.t[..., yv.coff + yv.C:]).all())
