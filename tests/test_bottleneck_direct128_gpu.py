"""The 128-plane fused bottleneck with its weights straight to registers (bottleneck_stream_direct128_kernel, FT_BNS_VARIANT128=3 on
large strips, =4 on small ones; blocks.py:105-120) vs the fp32 torch oracle and vs the ring kernel on the same strips
(FT_BNS_VARIANT128=1 / =2).  The two forms read the same weight stream and apply the same MFMAs to the same fp16 operands in the same
order (chunk by chunk, kk = 0..3, then the shift and residual MFMAs), so their outputs must be BIT-IDENTICAL: torch.equal, no bar.
Against the oracle the bar is the one of the other stream-kernel tests, 2e-2 x scale; the measured error is printed.
Measured on MI355X: 0.0000 % of the outputs differ between the forms on all nine shapes; max abs error against the oracle 3.5e-3 ..
8.1e-3 on scales of 8.5 .. 15.4 (both forms, the same figures)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd.hip_ops import ActView, FusedConv, record_bottleneck
from util import make_program, nchw_to_view, run_program, view_to_nchw

pytestmark = pytest.mark.gpu

P, C = 128, 512
RING_LARGE, RING_SMALL, DIRECT_LARGE, DIRECT_SMALL = 0, 5, 7, 8          # BnsPlan.variant (ft_bottleneck_stream_variant)
# what the rule picks for folded fp16 descriptors, per strip size (bns_plan: FT_BNS_DIRECT128_LARGE / _SMALL)
RULE_LARGE, RULE_SMALL = DIRECT_LARGE, DIRECT_SMALL

# (name, N, H, W, x channel stride, x channel offset, (ring, direct) values of FT_BNS_VARIANT128)
D128_CASES = [
    ("d128_r50_32x24", 3, 32, 24, 512, 0, (1, 3)),          # layer2 of R50 at 256 x 192: strips of 8 x 24 = 192 pixels on 240, first / interior / last
    ("d128_ragged_13x24", 2, 13, 24, 512, 0, (1, 3)),       # strips of 7 and 6 rows
    ("d128_view_offset_9x7", 1, 9, 7, 544, 32, (1, 3)),     # input is a channel slice of a wider buffer, neighbours poisoned
    ("d128_r101_48x36", 1, 48, 36, 512, 0, (1, 3)),         # layer2 of R101: 5-row strips, ragged 3-row last strip
    ("d128_r101_48x36_small", 1, 48, 36, 512, 0, (2, 4)),   # the same map on the small strips: 3 rows = 108 pixels on 180
    ("d128_tiny_5x3", 1, 5, 3, 512, 0, (1, 3)),             # one strip, mostly padding lanes
    ("d128_wide_6x60", 1, 6, 60, 512, 0, (1, 3)),           # 2-row strips of 120 pixels on 240
    ("d128_widest_3x85", 1, 3, 85, 512, 0, (1, 3)),         # the widest row of the large strips: 85 pixels on 255
    ("d128_recycle_b260", 260, 5, 3, 512, 0, (1, 3)),       # 260 workgroups: > 1 round on 256 CUs (LDS reuse across workgroups)
]


def _bn(seed, name, c):
    return {"weight": synth.uniform(seed, name + "g", (c,), 0.5, 1.5), "bias": synth.normal(seed, name + "b", (c,), 0.1),
            "running_mean": synth.normal(seed, name + "m", (c,), 0.1), "running_var": synth.uniform(seed, name + "v", (c,), 0.5, 1.5),
            "eps": 1e-5}


def _bnf(y, bn):
    return F.batch_norm(y, bn["running_mean"], bn["running_var"], bn["weight"], bn["bias"], training=False, eps=1e-5)


def _block(seed, name, P=128):
    C = 4 * P
    w1 = synth.normal(seed, name + ".w1", (P, C, 1, 1), std=(2.0 / C) ** 0.5)
    w2 = synth.normal(seed, name + ".w2", (P, P, 3, 3), std=(2.0 / (9 * P)) ** 0.5)
    w3 = synth.normal(seed, name + ".w3", (C, P, 1, 1), std=(2.0 / P) ** 0.5)
    return w1, w2, w3, _bn(seed, name + ".bn1", P), _bn(seed, name + ".bn2", P), _bn(seed, name + ".bn3", C)


def _oracle(x, w1, w2, w3, bn1, bn2, bn3):
    t1 = F.relu(_bnf(F.conv2d(x, w1), bn1))
    t2 = F.relu(_bnf(F.conv2d(t1, w2, padding=1), bn2))
    return F.relu(_bnf(F.conv2d(t2, w3), bn3) + x)


def _variant(prog):
    return int(_lib.load().ft_bottleneck_stream_variant(prog.calls[0][1][0]))


@pytest.mark.parametrize("case", D128_CASES, ids=[c[0] for c in D128_CASES])
def test_direct128_is_bit_identical_to_the_ring_kernel_and_matches_oracle(hip_lib, case, monkeypatch):
    name, N, H, W, xcs, xoff, forms = case
    dev, dtype, seed = torch.device("cuda:0"), torch.float16, 29
    w1, w2, w3, bn1, bn2, bn3 = _block(seed, name)
    x = synth.normal(seed, name + ".x", (N, C, H, W)).half().float()
    want = _oracle(x, w1, w2, w3, bn1, bn2, bn3)
    mk = dict(dtype=dtype, device=dev, act="relu")
    c1 = FusedConv(w1, bn=bn1, label="conv1", **mk)
    c2 = FusedConv(w2, pad=1, bn=bn2, label="conv2", **mk)
    c3 = FusedConv(w3, bn=bn3, label="conv3", **mk)
    xv = nchw_to_view(x, dtype, dev, cstride=xcs, coff=xoff)
    if xoff:
        xv.t[..., :xoff] = 7.0          # neighbours of the slice must not leak in
    ids = {1: RING_LARGE, 2: RING_SMALL, 3: DIRECT_LARGE, 4: DIRECT_SMALL}
    outs = {}
    for v in forms:                     # the same FusedConv layers (and the same weight stream) under both forms
        monkeypatch.setenv("FT_BNS_VARIANT128", str(v))
        y = ActView(torch.full((N, H, W, C + 32), 3.0, dtype=dtype, device=dev), C, 32)
        prog = make_program()
        record_bottleneck(prog, c1, c2, c3, xv, y, name)
        assert prog.calls[0][0] == "ft_bottleneck_stream_fwd"
        assert bool(prog.calls[0][1][0]._obj.folded)
        assert _variant(prog) == ids[v], f"{name}: FT_BNS_VARIANT128={v} plans variant {_variant(prog)}"
        run_program(prog)
        got = view_to_nchw(y)
        y.t.fill_(5.0)
        run_program(prog)
        assert torch.equal(view_to_nchw(y), got), f"{name} FT_BNS_VARIANT128={v}: two runs differ"
        assert torch.all(y.t[..., :32] == 5.0), "channels outside the output slice were written"
        outs[v] = got
    ring, direct = outs[forms[0]], outs[forms[1]]
    scale = max(1.0, want.abs().max().item())
    err_d, err_r = (direct - want).abs().max().item(), (ring - want).abs().max().item()
    diff = (direct - ring).abs()
    print(f"{name}: vs oracle max abs err direct {err_d:.3e} / ring {err_r:.3e} (scale {scale:.2f}); between the forms: "
          f"max {diff.max().item():.3e}, {100 * (diff > 0).float().mean().item():.4f} % of outputs differ")
    assert torch.equal(direct, ring), f"{name}: direct and ring forms differ (max {diff.max().item():.3e})"
    assert err_d <= 2e-2 * scale, f"{name}: direct form vs oracle max abs err {err_d:.3e} (scale {scale:.2f})"


def _desc(N, H, W, folded):
    d = _lib.BottleneckDesc()
    d.dtype = _lib.dtype_code(torch.float16)
    d.N, d.H, d.W, d.C, d.P = N, H, W, C, P
    d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = C, 0, C, 0
    d.folded = folded
    return d


def test_direct128_widest_row_is_planned_and_the_next_refused(hip_lib, monkeypatch):
    """W = 85 is the widest row whose one-row strip fits 256 halo pixels (3 x 85 = 255); W = 86 fits neither strip size.  Not launched."""
    lib = _lib.load()
    for v in ("0", "1", "3"):
        monkeypatch.setenv("FT_BNS_VARIANT128", v)
        assert int(lib.ft_bottleneck_stream_supported(ctypes.byref(_desc(1, 3, 85, 1)))) == _lib.FT_OK
        assert int(lib.ft_bottleneck_stream_supported(ctypes.byref(_desc(1, 3, 86, 1)))) == _lib.FT_ERR_UNSUPPORTED
        assert int(lib.ft_bottleneck_stream_variant(ctypes.byref(_desc(1, 3, 86, 1)))) == -1
    monkeypatch.setenv("FT_BNS_VARIANT128", "3")
    assert int(lib.ft_bottleneck_stream_variant(ctypes.byref(_desc(1, 3, 85, 1)))) == DIRECT_LARGE


def test_direct128_plan(hip_lib, monkeypatch):
    """bns_plan at 128 planes: the rule's choice for the benchmarked descriptor (64, 32, 24) (256 large strips: one round) and for R101
    at 16 crops (16, 48, 36) (256 small strips against 160 large ones); table-form descriptors keep the ring kernels; the forced values
    1-4 give their ids where the strips fit; the byte count and the stream layout never change."""
    lib = _lib.load()
    variant = lambda d: int(lib.ft_bottleneck_stream_variant(ctypes.byref(d)))
    layout = lambda d: int(lib.ft_bottleneck_stream_layout(ctypes.byref(d)))
    nbytes = lambda d: int(lib.ft_bottleneck_stream_weight_bytes(ctypes.byref(d)))
    shapes = [(64, 32, 24), (16, 48, 36)]
    monkeypatch.delenv("FT_BNS_VARIANT128", raising=False)
    assert variant(_desc(64, 32, 24, 1)) == RULE_LARGE and variant(_desc(64, 32, 24, 0)) == RING_LARGE
    assert variant(_desc(16, 48, 36, 1)) == RULE_SMALL and variant(_desc(16, 48, 36, 0)) == RING_SMALL
    monkeypatch.setenv("FT_BNS_VARIANT128", "0")
    assert variant(_desc(64, 32, 24, 1)) == RULE_LARGE and variant(_desc(16, 48, 36, 1)) == RULE_SMALL
    forced = {1: (RING_LARGE, RING_LARGE), 2: (RING_SMALL, RING_SMALL), 3: (DIRECT_LARGE, RING_LARGE), 4: (DIRECT_SMALL, RING_SMALL)}
    for v, (folded_id, table_id) in forced.items():
        monkeypatch.setenv("FT_BNS_VARIANT128", str(v))
        for shp in shapes:
            assert variant(_desc(*shp, 1)) == folded_id, f"FT_BNS_VARIANT128={v} {shp}: {variant(_desc(*shp, 1))}"
            assert variant(_desc(*shp, 0)) == table_id, f"FT_BNS_VARIANT128={v} {shp} table form: {variant(_desc(*shp, 0))}"
    # a row of 70 pixels fits no small strip (three halo rows are 210 pixels, the small strips hold 192): the forced small forms fall to
    # the large strips of their kernel; a row of 100 fits neither
    monkeypatch.setenv("FT_BNS_VARIANT128", "4")
    assert variant(_desc(1, 6, 100, 1)) == -1
    assert variant(_desc(1, 6, 70, 1)) == DIRECT_LARGE
    monkeypatch.setenv("FT_BNS_VARIANT128", "2")
    assert variant(_desc(1, 6, 70, 1)) == RING_LARGE
    for v in ("0", "1", "2", "3", "4"):
        monkeypatch.setenv("FT_BNS_VARIANT128", v)
        for shp in shapes:
            for folded in (0, 1):
                assert layout(_desc(*shp, folded)) == 0
                assert nbytes(_desc(*shp, folded)) == (8 + 18 + 8) * 16384


def test_direct128_folded_form_edge_cases(hip_lib, monkeypatch):
    """The operands of test_stream_folded_form_edge_cases (negative and zero gammas, shifts of a few hundred, a shift beyond the fp16
    range -> the table form on the ring kernel) at 128 planes with the direct form forced, judged as there: against the table form's
    own distance from the oracle."""
    monkeypatch.setenv("FT_BNS_VARIANT128", "3")
    N, H, W = 2, 32, 24
    dev, dtype, seed = torch.device("cuda:0"), torch.float16, 41
    name = f"fold_edge_{P}"
    w1 = synth.normal(seed, name + ".w1", (P, C, 1, 1), std=(2.0 / C) ** 0.5)
    w2 = synth.normal(seed, name + ".w2", (P, P, 3, 3), std=(2.0 / (9 * P)) ** 0.5)
    w3 = synth.normal(seed, name + ".w3", (C, P, 1, 1), std=(2.0 / P) ** 0.5)
    x = synth.normal(seed, name + ".x", (N, C, H, W)).half().float()
    for case in ("negative_gamma_big_shift", "shift_beyond_fp16"):
        bn1, bn2, bn3 = _bn(seed, name + ".bn1", P), _bn(seed, name + ".bn2", P), _bn(seed, name + ".bn3", C)
        sign = torch.where(synth.uniform(seed, name + ".sg", (P,)) < 0.4, -1.0, 1.0)
        bn1["weight"] = bn1["weight"] * sign
        bn2["weight"] = bn2["weight"] * torch.flip(sign, dims=[0])
        bn2["weight"][5] = 0.0
        bn3["weight"] = bn3["weight"] * torch.where(synth.uniform(seed, name + ".sg3", (C,)) < 0.5, -1.0, 1.0)
        bn3["bias"] = bn3["bias"] + synth.normal(seed, name + ".big", (C,), std=150.0)          # shifts of a few hundred on the output
        bn1["bias"][3] = 300.3
        if case == "shift_beyond_fp16":
            bn3["bias"][7] = 1.0e5
        want = _oracle(x, w1, w2, w3, bn1, bn2, bn3)
        mk = dict(dtype=dtype, device=dev, act="relu")
        c1, c2, c3 = FusedConv(w1, bn=bn1, **mk), FusedConv(w2, pad=1, bn=bn2, **mk), FusedConv(w3, bn=bn3, **mk)
        xv = nchw_to_view(x, dtype, dev)
        y = ActView(torch.zeros((N, H, W, C), dtype=dtype, device=dev), C, 0)
        prog = make_program()
        record_bottleneck(prog, c1, c2, c3, xv, y, name)
        assert prog.calls[0][0] == "ft_bottleneck_stream_fwd"
        folded = bool(prog.calls[0][1][0]._obj.folded)
        assert folded == (case != "shift_beyond_fp16"), f"{case}: folded = {folded}"
        assert _variant(prog) == (DIRECT_LARGE if folded else RING_LARGE), f"{case}: variant {_variant(prog)}"
        run_program(prog)
        got = view_to_nchw(y)
        fin = torch.isfinite(want) & (want.abs() < 6.0e4)                  # (the 1e5 channel overflows fp16 on every path)
        yt = ActView(torch.zeros((N, H, W, C), dtype=dtype, device=dev), C, 0)
        prog_t = make_program()
        record_bottleneck(prog_t, c1, c2, c3, xv, yt, name, fold=False)
        assert _variant(prog_t) == RING_LARGE
        run_program(prog_t)
        rel = lambda a: ((a - want).abs() / (1.0 + want.abs()))[fin]
        err, err_t = rel(got).max().item(), rel(view_to_nchw(yt)).max().item()
        print(f"{name} {case}: max relative err direct folded {err:.3e} / table form {err_t:.3e}; mean {rel(got).mean().item():.2e} / {rel(view_to_nchw(yt)).mean().item():.2e}")
        assert err <= 1.5 * err_t + 1e-3 and rel(got).mean().item() <= 1.5 * rel(view_to_nchw(yt)).mean().item() + 1e-5, f"{case}: folded {err:.3e} vs table {err_t:.3e}"
        if case == "shift_beyond_fp16":
            assert torch.isinf(got[:, 7]).all() and (got[:, 7] > 0).all()
