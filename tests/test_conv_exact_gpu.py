"""Bit-exact tests of the conv kernels on integer-valued data (tests/exact_cases.py): ft_conv_direct_fwd in every form, every tile
variant of ft_conv2d_fwd in fp16 and fp32, the forms with kernels of their own, the NCHW fp32 output form, the stem with the fused
max-pool, the fused tail and the K-concatenated shortcut conv.  Every product and every partial sum is exact and every stored value
is representable, so the output must EQUAL the float64 reference element for element: one product of +-1 dropped, doubled or taken
from the wrong place anywhere is a failure.  Each case names the form it ran, writes into a channel slice of a poisoned buffer and
(where the existing case does) reads from a channel slice whose neighbours are non-zero."""
import ctypes

import pytest
import torch

from flowtrack.pytorch_amd import hip_ops
from flowtrack.pytorch_amd.hip_ops import (ActView, FusedConv, FusedShortcutConv, act_stride, new_rowpacked_act, record_pack_input,
                                           round_up)
from util import make_program, run_program, view_to_nchw

import exact_cases as ec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
IGEMM_CALLS = ("ft_conv2d_fwd_ws", "ft_conv2d_fwd")


def _layer(c, ch, dtype, **kw):
    m = ch.meta
    return FusedConv(m["w"].float(), dtype=dtype, device=DEV, stride=c["s"], pad=c["p"], transposed=c["tr"], bias=m["bias"], bn=m["bn"],
                     act=c["act"], slope=ec.SLOPE if c["act"] == "leaky" else 0.0, label=c["name"], **kw)


def _hints(hip_lib, d):
    hints = (ctypes.c_int * 64)()
    n = hip_lib.ft_conv_tile_candidates(ctypes.byref(d), hints, 64)
    return [int(v) for v in hints[:n]]


def _hint_str(h):
    return f"hint {h:#x} ({hip_ops.tile_str(h)})"


def _use_direct(monkeypatch, mode):
    monkeypatch.setattr(hip_ops, "CONV_DIRECT", mode)
    monkeypatch.setattr(hip_ops, "_TILE_CACHE", {})


# ---- ft_conv_direct_fwd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.DIRECT_CONVS, ids=[c["name"] for c in ec.DIRECT_CONVS])
def test_direct_conv_is_exact(hip_lib, c, monkeypatch):
    """Every form of ft_conv_direct_fwd (the form is read back from ft_conv_direct_stream_id), and the implicit GEMM's default tile on
    the same views."""
    name = c["name"]
    ch = ec.conv_case(name)
    conv = _layer(c, ch, F16)
    (xcs, xoff), (ycs, yoff) = ec.direct_offsets(c)
    xv = ec.input_view(ch["x"], F16, DEV, cstride=xcs, coff=xoff)
    rv = ec.input_view(ch["r"], F16, DEV) if c["res"] else None
    want = ch["y"]
    N, Cout, Ho, Wo = want.shape
    for mode in (True, False):
        _use_direct(monkeypatch, mode)
        if c["k"] == 1:
            monkeypatch.setattr(hip_ops, "CONV_DIRECT_MAX_PIXELS", 1 << 20)
        y = ec.output_view(N, Ho, Wo, Cout, F16, DEV, ycs, yoff)
        prog = make_program()
        conv.record(prog, xv, y, residual=rv)
        prog.resolve_choices()      # recorded as [direct | implicit GEMM]: keep the first form
        assert prog.calls[0][0] == ("ft_conv_direct_fwd" if mode else "ft_conv2d_fwd_ws"), prog.calls[0][0]
        if mode:
            d = prog.conv_records[0][3]
            sid = int(hip_lib.ft_conv_direct_stream_id(d))
            assert ec.direct_form(sid, c["k"], c["tr"]) == c["form"], f"{name}: stream id {sid:#x}"
            assert hip_lib.ft_conv_direct_weight_bytes(d) == ec.direct_weight_bytes(c)
        run_program(prog)
        what = f"{name} ({c['form'] + ' form of ft_conv_direct_fwd' if mode else 'implicit GEMM'})"
        ec.assert_exact(view_to_nchw(y), want, what)
        ec.assert_guards(y, what)


@pytest.mark.parametrize("case", ec.DIRECT_SHORTCUT, ids=[c[0] for c in ec.DIRECT_SHORTCUT])
def test_direct_shortcut_conv_is_exact(hip_lib, case, monkeypatch):
    """conv3 + bn3 + projection shortcut + relu as one GEMM over K = [t2 | x]; both BN scales are folded into the fp16 weights, which
    powers of two survive unchanged."""
    name, N, Hx, Wx, planes, cin_x, s = case
    ch = ec.direct_shortcut_case(name)
    m = ch.meta
    fused = FusedShortcutConv(m["w3"].float(), m["bn3"], m["wd"].float(), m["bnd"], s, dtype=F16, device=DEV, act="relu", label=name)
    t2v = ec.input_view(ch["t2"], F16, DEV)
    xv = ec.input_view(ch["x"], F16, DEV, cstride=cin_x + 32, coff=32)
    want = ch["y"]
    _, cout, H, W = want.shape
    for mode in (True, False):
        _use_direct(monkeypatch, mode)
        monkeypatch.setattr(hip_ops, "CONV_DIRECT_MAX_PIXELS", 1 << 20)
        y = ec.output_view(N, H, W, cout, F16, DEV, cout + 64, 32)
        prog = make_program()
        fused.record(prog, t2v, xv, y)
        prog.resolve_choices()
        assert prog.calls[0][0] == ("ft_conv_direct_fwd" if mode else "ft_conv2d_fwd"), prog.calls[0][0]
        if mode:
            d = prog.conv_records[0][3]
            assert ec.direct_form(int(hip_lib.ft_conv_direct_stream_id(d)), 1, False) == "k1"
            assert hip_lib.ft_conv_direct_weight_bytes(d) == 2 * cout * (planes + cin_x)
        run_program(prog)
        what = f"{name} ({'direct' if mode else 'implicit GEMM'} shortcut conv)"
        ec.assert_exact(view_to_nchw(y), want, what)
        ec.assert_guards(y, what)


# ---- ft_conv2d_fwd --------------------------------------------------------------------------------------------------------------------
def _igemm_input(c, ch, dtype, layout="wide", prog=None):
    """The input view as the existing tests build it: row-packed for the small-Cin stems (through the library's own packer when `prog`
    is given), else NHWC with the networks' channel stride ("wide") or roundup8(Cin) ("tight")."""
    x = ch["x"]
    N, Cin, H, W = x.shape
    if Cin <= 16:
        xv = new_rowpacked_act(N, H, W, Cin, c["p"], dtype, DEV)
        if prog is not None:
            gx = x.float().to(DEV)
            record_pack_input(prog, gx, xv)
            prog.__dict__.setdefault("_exact_keep", []).append(gx)
        else:
            xv.t[:, :, xv.lpad:xv.lpad + W, :Cin] = x.permute(0, 2, 3, 1).to(device=DEV, dtype=dtype)
        return xv
    return ec.input_view(x, dtype, DEV, cstride=act_stride(Cin) if layout == "wide" else None)


def _guarded_out(N, Ho, Wo, Cout, dtype):
    return ec.output_view(N, Ho, Wo, Cout, dtype, DEV, round_up(Cout + 8, 8) + 8, 8)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("c", ec.VARIANT_CONVS, ids=[c["name"] for c in ec.VARIANT_CONVS])
def test_every_tile_variant_is_exact(hip_lib, c, dtype, monkeypatch):
    """Hint 0 and every hint of ft_conv_tile_candidates: each tile, halo-patch, stem-patch, 8-phase and split-K variant must give the
    very same (exact) result."""
    name = c["name"]
    _use_direct(monkeypatch, False)
    ch = ec.conv_case(name)
    layer = _layer(c, ch, dtype)
    want = ch["y"]
    N, Cout, Ho, Wo = want.shape
    xv = _igemm_input(c, ch, dtype)
    rv = ec.input_view(ch["r"], dtype, DEV) if c["res"] else None
    yv = _guarded_out(N, Ho, Wo, Cout, dtype)
    prog = make_program()
    layer.record(prog, xv, yv, residual=rv)
    assert [n for n, _ in prog.calls] in (["ft_conv2d_fwd_ws"], ["ft_conv2d_fwd"])
    d = prog.conv_records[0][3]
    hints = _hints(hip_lib, d)
    assert len(hints) >= 2, f"{name}: only {len(hints)} tile variants offered"
    if "splitk" in name:
        assert any(hip_ops.decode_tile(h).sk > 1 for h in hints), f"{name}: no split-K variant offered"
    if c.get("odd_splits") or name == "1x1_128_two_ktiles":
        mine = [h for h in hints if hip_ops.decode_tile(h).wide == hip_ops.WIDE8]
        assert mine or dtype != F16, f"{name}: the 8-phase tile is not offered"
        if c.get("odd_splits") and mine:      # the odd K splits (3, 5, 6, 7 slices) forced onto the 8-phase tile, as test_conv8_gpu.py does
            assert any(hip_ops.decode_tile(h).sk > 1 for h in mine), f"{name}: no split-K form of the 8-phase tile offered"
            assert any(hip_ops.decode_tile(h).sk == 1 for h in mine)
            hints = hints + [hip_ops.encode_tile(bp=256, bc=256, ks=1, wide=hip_ops.WIDE8, sk=sk) for sk in (3, 5, 6, 7)]
    for h in [0] + hints:
        d.tile_hint = h
        yv.t.fill_(ec.Y_POISON)
        run_program(prog)
        what = f"{name} {dtype} {_hint_str(h)}"
        ec.assert_exact(view_to_nchw(yv), want, what)
        ec.assert_guards(yv, what)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("c", ec.OWN_KERNEL_CONVS, ids=[c["name"] for c in ec.OWN_KERNEL_CONVS])
def test_forms_with_their_own_kernels_are_exact(hip_lib, c, dtype, monkeypatch):
    """Few output channels, the predict_flow patch / matrix-pipe kernels, the persistent stem through the library's packer, a ragged
    Cin in the tight layout; on two of them the NCHW fp32 output form as well."""
    name = c["name"]
    _use_direct(monkeypatch, False)
    ch = ec.conv_case(name)
    layer = _layer(c, ch, dtype)
    want = ch["y"]
    N, Cout, Ho, Wo = want.shape
    prog = make_program()
    xv = _igemm_input(c, ch, dtype, c.get("layout", "wide"), prog if c.get("packer") else None)
    rv = ec.input_view(ch["r"], dtype, DEV) if c["res"] else None
    yv = _guarded_out(N, Ho, Wo, Cout, dtype)
    layer.record(prog, xv, yv, residual=rv)
    y_nchw = None
    if c.get("nchw_too"):
        y_nchw = torch.full((N, Cout, Ho, Wo), 5.0, dtype=torch.float32, device=DEV)
        layer.record(prog, xv, y_nchw, residual=rv)
    assert all(n in IGEMM_CALLS for n, _ in prog.calls if is_conv(n)), [n for n, _ in prog.calls]
    run_program(prog)
    ec.assert_exact(view_to_nchw(yv), want, f"{name} {dtype}")
    ec.assert_guards(yv, name)
    if y_nchw is not None:
        ec.assert_exact(y_nchw, want, f"{name} {dtype} NCHW fp32 output")
    if c.get("packer"):
        W = ch["x"].shape[3]
        assert torch.all(xv.t[:, :, :xv.lpad] == 0) and torch.all(xv.t[:, :, xv.lpad + W:] == 0) and torch.all(xv.t[..., c["Cin"]:] == 0)


def is_conv(name):
    return hip_ops.is_conv_call(name)


@pytest.mark.parametrize("case", ec.STEM_POOL, ids=[c[0] for c in ec.STEM_POOL])
def test_stem_with_fused_maxpool_is_exact(hip_lib, case):
    """conv1 -> bn1 -> relu -> maxpool in one launch, from the packed input and from the NCHW fp32 input itself."""
    name, N, H, W = case
    ch = ec.stem_pool_case(name)
    m = ch.meta
    layer = FusedConv(m["w"].float(), stride=2, pad=3, bn=m["bn"], act="relu", dtype=F16, device=DEV, label=name)
    xs = ch["x"].float().to(DEV)
    want = ch["y"]
    Hp, Wp = H // 4, W // 4
    assert tuple(want.shape) == (N, 64, Hp, Wp)
    fused_in = new_rowpacked_act(N, H, W, 3, 5, F16, DEV)
    pooled = ec.output_view(N, Hp, Wp, 64, F16, DEV, 96, 16)
    prog = make_program()
    record_pack_input(prog, xs, fused_in)
    layer.record(prog, fused_in, pooled, pool=True)
    assert [n for n, _ in prog.calls if is_conv(n)] in (["ft_conv2d_fwd_ws"], ["ft_conv2d_fwd"]) and prog.conv_records[-1][3].pool == 1
    run_program(prog)
    ec.assert_exact(view_to_nchw(pooled), want, f"{name}: stem + max-pool on the packed input")
    ec.assert_guards(pooled, name)
    planar = ec.output_view(N, Hp, Wp, 64, F16, DEV, 96, 16)
    geom = new_rowpacked_act(N, H, W, 3, 5, F16, "meta")
    prog3 = make_program()
    layer.record(prog3, geom, planar, pool=True, x_nchw=xs)
    assert [n for n, _ in prog3.calls if is_conv(n)] in (["ft_conv2d_fwd_ws"], ["ft_conv2d_fwd"]) and prog3.conv_records[-1][3].x_nchw_f32 == 1
    run_program(prog3)
    ec.assert_exact(view_to_nchw(planar), want, f"{name}: stem + max-pool on the NCHW fp32 input")
    ec.assert_guards(planar, name)


@pytest.mark.parametrize("nchw", [True, False], ids=["nchw_f32", "nhwc_f16"])
@pytest.mark.parametrize("case", ec.TAILS, ids=[c[0] for c in ec.TAILS])
def test_fused_tail_is_exact(hip_lib, case, nchw, monkeypatch):
    """Wt . relu(bn(conv(x))) + bt in one launch with integer tail weights (their lo halves are zero), on every tile the library offers
    (the 128-pixel tile and, at 256 channels, the 8-phase tile)."""
    name, N, Cin, H, W, Cout, k, stride, pad, transposed, nt = case
    _use_direct(monkeypatch, False)
    ch = ec.tail_case(name)
    m = ch.meta
    layer = FusedConv(m["w"].float(), dtype=F16, device=DEV, stride=stride, pad=pad, transposed=transposed, bn=m["bn"], act="relu", label=name,
                      tail_weight=m["wt"].float(), tail_bias=m["bt"].float())
    want = ch["y"]
    _, _, Ho, Wo = want.shape
    xv = ec.input_view(ch["x"], F16, DEV, cstride=act_stride(Cin))
    prog = make_program()
    if nchw:
        y = torch.full((N, nt, Ho, Wo), 5.0, dtype=torch.float32, device=DEV)
    else:
        y = ec.output_view(N, Ho, Wo, nt, F16, DEV, 40, 4)
    layer.record(prog, xv, y)
    assert [n for n, _ in prog.calls] in (["ft_conv2d_fwd_ws"], ["ft_conv2d_fwd"])
    d = prog.conv_records[-1][3]
    assert d.tail_cout == nt
    hints = _hints(hip_lib, d)
    if Cout == 256:
        assert len(hints) == 2 and sum(hip_ops.decode_tile(h).wide == hip_ops.WIDE8 for h in hints) == 1, "a 256-channel tail layer offers the 128-pixel default and the 8-phase tile"
    for h in [0] + hints:
        d.tile_hint = h
        (y if nchw else y.t).fill_(5.0 if nchw else ec.Y_POISON)
        run_program(prog)
        what = f"{name} {'NCHW fp32' if nchw else 'NHWC fp16'} {_hint_str(h)}"
        ec.assert_exact(y if nchw else view_to_nchw(y), want, what)
        if not nchw:
            ec.assert_guards(y, what)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", ec.SHORTCUTS, ids=[c[0] for c in ec.SHORTCUTS])
def test_fused_shortcut_conv_is_exact(hip_lib, case, dtype, monkeypatch):
    """relu(bn3(conv3(t2)) + bn_d(conv_d(x))) on the implicit GEMM, every tile variant, one shape per stride."""
    name, N, planes, cin, H, W, s = case
    _use_direct(monkeypatch, False)
    ch = ec.shortcut_case(name)
    m = ch.meta
    layer = FusedShortcutConv(m["w3"].float(), m["bn3"], m["wd"].float(), m["bnd"], s, dtype=dtype, device=DEV, label=name)
    want = ch["y"]
    _, cout, Ho, Wo = want.shape
    t2v = ec.input_view(ch["t2"], dtype, DEV, cstride=act_stride(planes))
    xv = ec.input_view(ch["x"], dtype, DEV, cstride=act_stride(cin) + 32, coff=32)
    yv = _guarded_out(N, Ho, Wo, cout, dtype)
    prog = make_program()
    layer.record(prog, t2v, xv, yv)
    assert [n for n, _ in prog.calls] == ["ft_conv2d_fwd"]
    d = prog.conv_records[0][3]
    hints = _hints(hip_lib, d)
    assert len(hints) >= 2
    for h in [0] + hints:
        assert h == 0 or (hip_ops.decode_tile(h).ks == 1 and not hip_ops.decode_tile(h).halo), "K-concat offers no split-K / halo variants"
        d.tile_hint = h
        yv.t.fill_(ec.Y_POISON)
        run_program(prog)
        what = f"{name} {dtype} {_hint_str(h)}"
        ec.assert_exact(view_to_nchw(yv), want, what)
        ec.assert_guards(yv, what)
