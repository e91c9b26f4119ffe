"""Bit-exact tests of the fused bottleneck entry points on integer-valued data (tests/exact_cases.py): t1, t2 and y are integers (or
half-integers) that fp16 holds exactly, every BatchNorm scale is +-1 or +-0.5 and every shift a small (half-)integer, so the table
forms, the forms that fold the scale into fp16 weights and add the shift and the residual by MFMA, and every strip / tile / cluster
variant must EQUAL the float64 reference element for element.  Each case asserts the entry point and the form it ran, writes into a
channel slice of a poisoned buffer and, where the existing case does, reads from a slice with non-zero neighbours."""
import ctypes

import pytest
import torch

from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd.hip_ops import (FusedConv, FusedShortcutConv, _bottleneck_desc, bottleneck_cluster_supported,
                                           bottleneck_entry_fusable, bottleneck_exit_fusable, bottleneck_fusable, bottleneck_head_fusable,
                                           bottleneck_head_stream_fusable, bottleneck_strips_supported, record_bottleneck,
                                           record_bottleneck_entry, record_bottleneck_exit, record_bottleneck_head,
                                           record_bottleneck_head_stream)
from util import make_program, run_program, view_to_nchw

import exact_cases as ec

pytestmark = pytest.mark.gpu

DEV, F16 = torch.device("cuda:0"), torch.float16
RING_LARGE, RING_SMALL, DIRECT_LARGE, DIRECT_SMALL = 0, 5, 7, 8          # BnsPlan.variant at 128 planes (ft_bottleneck_stream_variant), as test_bottleneck_direct128_gpu.py
KNOBS = ("FT_BNS_VARIANT", "FT_BNS_VARIANT128", "FT_BNS_WAVES", "FT_BNK_RSTAT", "FT_BNR_SR")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _convs(ch, stride2=1):
    m = ch.meta
    mk = dict(dtype=F16, device=DEV, act="relu")
    c1 = FusedConv(m["w1"].float(), bn=m["bn1"], label="conv1", **mk)
    c2 = FusedConv(m["w2"].float(), stride=stride2, pad=1, bn=m["bn2"], label="conv2", **mk)
    c3 = FusedConv(m["w3"].float(), bn=m["bn3"], label="conv3", **mk) if "w3" in m and "wd" not in m else None
    return c1, c2, c3


def _x(ch, xcs, xoff):
    return ec.input_view(ch["x"], F16, DEV, cstride=xcs, coff=xoff)


def _y(want, pad=32):
    N, C, H, W = want.shape
    return ec.output_view(N, H, W, C, F16, DEV, C + 2 * pad, pad)


def _desc(prog):
    return prog.calls[0][1][0]._obj


def _check(prog, y, want, what, entry):
    assert [n for n, _ in prog.calls] == [entry], f"{what}: launched {[n for n, _ in prog.calls]}"
    run_program(prog)
    ec.assert_exact(view_to_nchw(y), want, what)
    ec.assert_guards(y, what)


@pytest.mark.parametrize("case", ec.PATCH_BLOCKS, ids=[c[0] for c in ec.PATCH_BLOCKS])
def test_patch_form_is_exact(hip_lib, case):
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    assert bottleneck_fusable(c1, c2, c3, xv, y)
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, form="patch")
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_fwd", "ft_bottleneck_fwd")


@pytest.mark.parametrize("case", ec.RSTAT_BLOCKS, ids=[c[0] for c in ec.RSTAT_BLOCKS])
def test_register_stationary_strip_form_is_exact(hip_lib, case, monkeypatch):
    """The strip form folds each scale into its fp16 weights and adds shift and residual inside the matrix product."""
    name, N, H, W, xcs, xoff, P, sr = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    monkeypatch.setenv("FT_BNK_RSTAT", "2")
    monkeypatch.setenv("FT_BNR_SR", str(sr))
    assert bottleneck_strips_supported(xv, y, P)
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, form="strips")
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_rstat_fwd, {sr} rows per strip", "ft_bottleneck_rstat_fwd")


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "tables"])
@pytest.mark.parametrize("strips", [1, 2], ids=["large_strips", "small_strips"])
@pytest.mark.parametrize("case", ec.S128_BLOCKS, ids=[c[0] for c in ec.S128_BLOCKS])
def test_stream_128_is_exact(hip_lib, case, strips, fold, monkeypatch):
    """The ring kernel of the 128-plane block on both strip sizes (FT_BNS_VARIANT128 = 1 / 2), folded operands and tables."""
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    monkeypatch.setenv("FT_BNS_VARIANT128", str(strips))
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, fold=fold)
    assert bool(_desc(prog).folded) == fold
    v = int(hip_lib.ft_bottleneck_stream_variant(prog.calls[0][1][0]))
    assert v == {1: RING_LARGE, 2: RING_SMALL}[strips], f"{name}: FT_BNS_VARIANT128={strips} plans variant {v}"
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_stream_fwd variant {v}, folded {fold}", "ft_bottleneck_stream_fwd")


@pytest.mark.parametrize("forced", [3, 4], ids=["large_strips", "small_strips"])
@pytest.mark.parametrize("case", ec.D128_BLOCKS, ids=[c[0] for c in ec.D128_BLOCKS])
def test_direct128_form_is_exact(hip_lib, case, forced, monkeypatch):
    """FT_BNS_VARIANT128 = 3 / 4: the weights-straight-to-registers kernel on the large / small strips (folded operands only)."""
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    monkeypatch.setenv("FT_BNS_VARIANT128", str(forced))
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name)
    assert bool(_desc(prog).folded)
    v = int(hip_lib.ft_bottleneck_stream_variant(prog.calls[0][1][0]))
    assert v == {3: DIRECT_LARGE, 4: DIRECT_SMALL}[forced], f"{name}: FT_BNS_VARIANT128={forced} plans variant {v}"
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_stream_fwd variant {v}", "ft_bottleneck_stream_fwd")


def _s256_params():
    out = []
    for case in ec.S256_BLOCKS:
        for variant in (2, 3):
            if variant == 2 and case[2] * case[3] > 64 and case[3] > 32:
                continue            # full-width strips need a row of <= 32 pixels at 256 planes
            out.append(pytest.param(case, variant, id=f"{case[0]}-{'full_width_strips' if variant == 2 else 'column_split'}"))
    return out


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "tables"])
@pytest.mark.parametrize("case, variant", _s256_params())
def test_stream_256_variants_are_exact(hip_lib, case, variant, fold, monkeypatch):
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    monkeypatch.setenv("FT_BNS_VARIANT", str(variant))
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, fold=fold)
    assert bool(_desc(prog).folded) == fold
    assert int(hip_lib.ft_bottleneck_stream_layout(prog.calls[0][1][0])) == 0
    assert int(hip_lib.ft_bottleneck_stream_variant(prog.calls[0][1][0])) == variant
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_stream_fwd FT_BNS_VARIANT={variant}, folded {fold}", "ft_bottleneck_stream_fwd")


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "tables"])
@pytest.mark.parametrize("variant", [2, 3], ids=["full_width_strips", "column_split"])
@pytest.mark.parametrize("case", ec.S256_BLOCKS[:2], ids=[c[0] for c in ec.S256_BLOCKS[:2]])
def test_stream_256_eight_wave_form_is_exact(hip_lib, case, variant, fold, monkeypatch):
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    monkeypatch.setenv("FT_BNS_VARIANT", str(variant))
    monkeypatch.setenv("FT_BNS_WAVES", "8")
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, fold=fold)
    assert bool(_desc(prog).folded) == fold
    assert int(hip_lib.ft_bottleneck_stream_variant(prog.calls[0][1][0])) == variant
    _check(prog, y, ch["y"], f"{name}: eight-wave form, FT_BNS_VARIANT={variant}, folded {fold}", "ft_bottleneck_stream_fwd")


@pytest.mark.parametrize("case", ec.T16_BLOCKS, ids=[c[0] for c in ec.T16_BLOCKS])
def test_tile16_form_is_exact(hip_lib, case, monkeypatch):
    """FT_BNS_VARIANT=6: 16-pixel MFMA tiles; the form exists for the folded operands only."""
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    monkeypatch.setenv("FT_BNS_VARIANT", "6")
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, fold=True)
    assert bool(_desc(prog).folded)
    assert int(hip_lib.ft_bottleneck_stream_layout(prog.calls[0][1][0])) == 1, f"{name}: FT_BNS_VARIANT=6 did not plan the 16-pixel form"
    _check(prog, y, ch["y"], f"{name}: 16-pixel form", "ft_bottleneck_stream_fwd")


@pytest.mark.parametrize("case", ec.CLUSTER_BLOCKS, ids=[c[0] for c in ec.CLUSTER_BLOCKS])
def test_cluster_form_is_exact(hip_lib, case):
    """Four workgroups per image exchange t1 / t2 inside the launch: exact on the first run and on a second one with poisoned exchange
    buffers, and the status word stays 0 (no hand-off timed out)."""
    name, N, H, W, xcs, xoff, P = case
    ch = ec.block_case(name)
    c1, c2, c3 = _convs(ch)
    xv, y = _x(ch, xcs, xoff), _y(ch["y"])
    assert bottleneck_cluster_supported(xv, y, P)
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y, name, cluster=True)
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_cluster_fwd", "ft_bottleneck_cluster_fwd")
    ws = prog._cluster_ws[(N, H, W)]
    soff = int(_lib.load().ft_bottleneck_cluster_status_offset(ctypes.byref(_bottleneck_desc(xv, y, P))))
    y.t[..., y.coff:y.coff + y.C].fill_(5.0)
    ws[:soff - 64 * ((N + 7) // 8 * 8)].fill_(0x3C)       # poison the exchange buffers (not the counters)
    run_program(prog)
    ec.assert_exact(view_to_nchw(y), ch["y"], f"{name}: second run of the cluster form")
    ec.assert_guards(y, name)
    assert int(ws[soff:soff + 4].view(torch.int32).item()) == 0, "a cluster hand-off timed out"


def test_head_only_form_is_exact(hip_lib):
    name, N, H, W = ec.HEAD_BLOCK
    ch = ec.block_case("head." + name)
    c1, c2, _ = _convs(ch)
    xv, t2 = _x(ch, None, 0), _y(ch["t2"])
    assert bottleneck_head_fusable(c1, c2, xv, t2)
    prog = make_program()
    record_bottleneck_head(prog, c1, c2, xv, t2, name)
    assert _desc(prog).head_only == 1
    _check(prog, t2, ch["t2"], f"{name}: ft_bottleneck_fwd (head only)", "ft_bottleneck_fwd")


def test_stream_head_stride2_is_exact(hip_lib, monkeypatch):
    name, N, H, W, xcs, xoff = ec.HEAD2_BLOCK
    ch = ec.block_case("head2." + name)
    c1, c2, _ = _convs(ch, stride2=2)
    for waves in (4, 8):
        monkeypatch.setenv("FT_BNS_WAVES", str(waves))
        xv, t2 = _x(ch, xcs + 32, 32), _y(ch["t2"])
        assert bottleneck_head_stream_fusable(c1, c2, xv, t2)
        prog = make_program()
        record_bottleneck_head_stream(prog, c1, c2, xv, t2, name)
        assert _desc(prog).head_only == 1 and _desc(prog).stride == 2
        _check(prog, t2, ch["t2"], f"{name}: ft_bottleneck_stream_fwd (head only, stride 2, {waves} waves)", "ft_bottleneck_stream_fwd")


def test_entry_block_is_exact(hip_lib):
    name, N, H, W = ec.ENTRY_BLOCK
    ch = ec.block_case("entry." + name)
    m = ch.meta
    c1, c2, _ = _convs(ch)
    sc = FusedShortcutConv(m["w3"].float(), m["bn3"], m["wd"].float(), m["bnd"], 1, dtype=F16, device=DEV, act="relu", label="conv3+downsample")
    xv, y = _x(ch, None, 0), _y(ch["y"])
    assert bottleneck_entry_fusable(c1, c2, sc, xv, y)
    prog = make_program()
    record_bottleneck_entry(prog, c1, c2, sc, xv, y, name)
    assert _desc(prog).projection == 1
    _check(prog, y, ch["y"], f"{name}: ft_bottleneck_fwd (projection)", "ft_bottleneck_fwd")


@pytest.mark.parametrize("case", ec.EXIT_BLOCKS, ids=[c[0] for c in ec.EXIT_BLOCKS])
def test_exit_form_is_exact(hip_lib, case):
    """The block and the next stage's opening 1x1 conv in one launch: t1 of the next stage everywhere, y at the even pixels."""
    name, N, H, W, xcs, xoff, _, _, mode = case
    ch = ec.block_case("exit." + name)
    m = ch.meta
    c1, c2, c3 = _convs(ch)
    tail = FusedConv(m["wt"].float(), bn=m["bnt"], label="tail", dtype=F16, device=DEV, act="relu")
    want_y, want_t1 = ch["y"][:, :, ::2, ::2].contiguous(), ch["n1"]
    xv, yv, t1v = _x(ch, xcs, xoff), _y(want_y), _y(want_t1)
    assert bottleneck_exit_fusable(c1, c2, c3, tail, xv, yv, t1v, mode)
    prog = make_program()
    record_bottleneck_exit(prog, c1, c2, c3, tail, xv, yv, t1v, name, mode)
    _check(prog, t1v, want_t1, f"{name}: t1 of ft_bottleneck_exit_fwd", "ft_bottleneck_exit_fwd")
    ec.assert_exact(view_to_nchw(yv), want_y, f"{name}: y (even pixels) of ft_bottleneck_exit_fwd")
    ec.assert_guards(yv, name)
