"""The 256-plane fused bottleneck on 16-pixel MFMA tiles (bottleneck_stream_tile16_kernel, FT_BNS_VARIANT=6; blocks.py:105-120) vs the
fp32 torch oracle and vs the forced 32-pixel full-width-strip form (FT_BNS_VARIANT=2).  The two forms multiply the same fp16 operands
(weights with the scale folded in, shift pairs, t1 / t2 rounded to fp16); a K32 MFMA sums 32 products where two K16 ones summed
16 + 16, so fp32 sums may differ in their last bits and a few fp16 roundings may flip: the bars are those of
test_stream_256_variants_match_oracle_and_each_other; the fraction of differing elements is printed, not asserted.
Measured on MI355X: 0.00 % of the elements differ on all seven shapes (max abs error against the oracle 4.2e-3 .. 8.8e-3 on scales
of 10.6 .. 15.8, the 32-pixel form's own figures): the K32 instruction adds its 8-wide k groups in the order two K16 ones do."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd.hip_ops import ActView, FusedConv, record_bottleneck
from util import make_program, nchw_to_view, run_program, view_to_nchw

pytestmark = pytest.mark.gpu

# (name, N, H, W, x channel stride, x channel offset): 256-plane maps whose strips fit 48 output pixels on 80 halo pixels
T16_CASES = [
    ("t16_r50_16x12_b5", 5, 16, 12, 1024, 0),          # layer3 of R50 at 256 x 192: four strips of 4 x 12 per image, three full tiles
    ("t16_r50_16x12_b64", 64, 16, 12, 1024, 0),        # the benchmarked batch: 256 workgroups, one per CU
    ("t16_ragged_9x7", 3, 9, 7, 1024, 0),              # 5-row strips on 9 rows: the last strip has 4 rows, 35 / 28 pixels in 3 tiles
    ("t16_view_offset_9x7", 1, 9, 7, 1056, 32),        # input is a channel slice of a wider buffer
    ("t16_r101_24x18", 2, 24, 18, 1024, 0),            # layer3 of R101: strips of 2 x 18 = 36 pixels on 72
    ("t16_tiny_5x3", 1, 5, 3, 1024, 0),                # one strip, mostly padding lanes
    ("t16_recycle_b100", 100, 16, 12, 1024, 0),        # 400 workgroups: > 1 round on 256 CUs (LDS reuse across workgroups)
]


def _bn(seed, name, c):
    return {"weight": synth.uniform(seed, name + "g", (c,), 0.5, 1.5), "bias": synth.normal(seed, name + "b", (c,), 0.1),
            "running_mean": synth.normal(seed, name + "m", (c,), 0.1), "running_var": synth.uniform(seed, name + "v", (c,), 0.5, 1.5),
            "eps": 1e-5}


def _bnf(y, bn):
    return F.batch_norm(y, bn["running_mean"], bn["running_var"], bn["weight"], bn["bias"], training=False, eps=1e-5)


def _block(seed, name, P=256):
    C = 4 * P
    w1 = synth.normal(seed, name + ".w1", (P, C, 1, 1), std=(2.0 / C) ** 0.5)
    w2 = synth.normal(seed, name + ".w2", (P, P, 3, 3), std=(2.0 / (9 * P)) ** 0.5)
    w3 = synth.normal(seed, name + ".w3", (C, P, 1, 1), std=(2.0 / P) ** 0.5)
    return w1, w2, w3, _bn(seed, name + ".bn1", P), _bn(seed, name + ".bn2", P), _bn(seed, name + ".bn3", C)


def _oracle(x, w1, w2, w3, bn1, bn2, bn3):
    t1 = F.relu(_bnf(F.conv2d(x, w1), bn1))
    t2 = F.relu(_bnf(F.conv2d(t1, w2, padding=1), bn2))
    return F.relu(_bnf(F.conv2d(t2, w3), bn3) + x)


def _layout(prog):
    return int(_lib.load().ft_bottleneck_stream_layout(prog.calls[0][1][0]))


@pytest.mark.parametrize("case", T16_CASES, ids=[c[0] for c in T16_CASES])
def test_tile16_matches_oracle_and_the_32_pixel_form(hip_lib, case, monkeypatch):
    name, N, H, W, xcs, xoff = case
    C = 1024
    dev, dtype, seed = torch.device("cuda:0"), torch.float16, 23
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
    outs = {}
    for v in (6, 2):                    # the same FusedConv layers under both forms: the stream must be re-packed, not reused
        monkeypatch.setenv("FT_BNS_VARIANT", str(v))
        y = ActView(torch.full((N, H, W, C + 32), 3.0, dtype=dtype, device=dev), C, 32)
        prog = make_program()
        record_bottleneck(prog, c1, c2, c3, xv, y, name)
        assert prog.calls[0][0] == "ft_bottleneck_stream_fwd"
        assert bool(prog.calls[0][1][0]._obj.folded)
        assert _layout(prog) == (1 if v == 6 else 0), f"{name}: FT_BNS_VARIANT={v} plans stream layout {_layout(prog)}"
        run_program(prog)
        got = view_to_nchw(y)
        y.t.fill_(5.0)
        run_program(prog)
        assert torch.equal(view_to_nchw(y), got), f"{name} variant {v}: two runs differ"
        assert torch.all(y.t[..., :32] == 5.0), "channels outside the output slice were written"
        outs[v] = got
    scale = max(1.0, want.abs().max().item())
    err = {v: (outs[v] - want).abs().max().item() for v in outs}
    diff = (outs[6] - outs[2]).abs()
    print(f"{name}: vs oracle max abs err 16-pixel form {err[6]:.3e} / 32-pixel form {err[2]:.3e} (scale {scale:.2f}); between the forms: "
          f"max {diff.max().item():.3e}, mean {diff.mean().item():.2e}, {100 * (diff > 0).float().mean().item():.2f} % of outputs differ")
    assert err[6] <= 2e-2 * scale, f"{name}: 16-pixel form vs oracle max abs err {err[6]:.3e} (scale {scale:.2f})"
    assert diff.max().item() <= 1e-2 * scale, f"{name}: 16-pixel vs 32-pixel form max abs diff {diff.max().item():.3e}"


def test_tile16_stream_is_repacked_per_layout(hip_lib, monkeypatch):
    """One set of FusedConv layers recorded under the 32-pixel form, then under the 16-pixel form, then under both again: every program
    reads a stream in its own fragment order (the cache key carries ft_bottleneck_stream_layout), so each output is within the bars,
    and the programs recorded first still are after the other layout was packed."""
    name, N, H, W = "t16_layout", 3, 16, 12
    C = 1024
    dev, dtype, seed = torch.device("cuda:0"), torch.float16, 31
    w1, w2, w3, bn1, bn2, bn3 = _block(seed, name)
    x = synth.normal(seed, name + ".x", (N, C, H, W)).half().float()
    want = _oracle(x, w1, w2, w3, bn1, bn2, bn3)
    scale = max(1.0, want.abs().max().item())
    mk = dict(dtype=dtype, device=dev, act="relu")
    c1, c2, c3 = FusedConv(w1, bn=bn1, **mk), FusedConv(w2, pad=1, bn=bn2, **mk), FusedConv(w3, bn=bn3, **mk)
    xv = nchw_to_view(x, dtype, dev)
    progs = []
    for v in (2, 6, 2, 6):
        monkeypatch.setenv("FT_BNS_VARIANT", str(v))
        y = ActView(torch.zeros((N, H, W, C), dtype=dtype, device=dev), C, 0)
        prog = make_program()
        record_bottleneck(prog, c1, c2, c3, xv, y, name)
        assert _layout(prog) == (1 if v == 6 else 0)
        progs.append((v, prog, y))
    streams = {v: {p.calls[0][1][2] for u, p, _ in progs if u == v} for v in (2, 6)}     # the weight-stream pointers of the launches
    assert len(streams[2]) == 1 and len(streams[6]) == 1 and not (streams[2] & streams[6]), "one stream per layout, never shared"
    outs = {}
    for v, prog, y in progs:
        monkeypatch.setenv("FT_BNS_VARIANT", str(v))
        run_program(prog)
        got = view_to_nchw(y)
        err = (got - want).abs().max().item()
        assert err <= 2e-2 * scale, f"variant {v}: vs oracle max abs err {err:.3e} (scale {scale:.2f})"
        assert v not in outs or torch.equal(outs[v], got), f"variant {v}: the second program differs from the first"
        outs[v] = got
    assert (outs[6] - outs[2]).abs().max().item() <= 1e-2 * scale


def test_tile16_is_the_default_where_it_costs_less(hip_lib, monkeypatch):
    """bns_plan: folded fp16 descriptors whose strips fit take the 16-pixel form where rounds x MFMA cycles are lowest (the R50 batch-64
    step); table-form descriptors, FT_BNS_WAVES=8 and the forced variants keep the 32-pixel kernels; the byte count never changes."""
    lib = _lib.load()
    monkeypatch.delenv("FT_BNS_VARIANT", raising=False)
    monkeypatch.delenv("FT_BNS_WAVES", raising=False)

    def desc(N, H, W, folded):
        d = _lib.BottleneckDesc()
        d.dtype = _lib.dtype_code(torch.float16)
        d.N, d.H, d.W, d.C, d.P = N, H, W, 1024, 256
        d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = 1024, 0, 1024, 0
        d.folded = folded
        return d
    layout = lambda d: int(lib.ft_bottleneck_stream_layout(ctypes.byref(d)))
    nbytes = lambda d: int(lib.ft_bottleneck_stream_weight_bytes(ctypes.byref(d)))
    assert layout(desc(64, 16, 12, 1)) == 1           # 256 strips either way: one round of 472 units instead of 608
    assert layout(desc(48, 16, 12, 1)) == 1           # 192 strips: one round of 472 against 608, 880 and the column split's 2 x 336
    assert layout(desc(32, 16, 12, 1)) == 0           # 256 column halves fill one round at 336
    assert layout(desc(128, 16, 12, 1)) == 0          # 512 strips = two rounds (944) against ONE round of 256 8-row strips (880)
    assert layout(desc(64, 16, 12, 0)) == 0
    assert layout(desc(16, 24, 18, 1)) == 0           # R101 at 16 crops: the column-split form keeps the shape
    assert layout(desc(64, 6, 60, 1)) == 0            # a row of 60 pixels fits no 48-pixel strip
    assert nbytes(desc(64, 16, 12, 1)) == nbytes(desc(64, 16, 12, 0)) == (16 + 36 + 16) * 32768
    monkeypatch.setenv("FT_BNS_WAVES", "8")
    assert layout(desc(64, 16, 12, 1)) == 0
    monkeypatch.delenv("FT_BNS_WAVES")
    for v in ("1", "2", "3"):
        monkeypatch.setenv("FT_BNS_VARIANT", v)
        assert layout(desc(64, 16, 12, 1)) == 0
    monkeypatch.setenv("FT_BNS_VARIANT", "6")
    assert layout(desc(2, 16, 12, 1)) == 1 and layout(desc(2, 16, 12, 0)) == 0 and layout(desc(2, 6, 60, 1)) == 0


def test_tile16_folded_form_edge_cases(hip_lib, monkeypatch):
    """The operands of test_stream_folded_form_edge_cases (negative and zero gammas, shifts of a few hundred, a shift beyond the fp16
    range -> the table form) with the 16-pixel form forced, judged as there: against the table form's own distance from the oracle."""
    monkeypatch.setenv("FT_BNS_VARIANT", "6")
    P, C = 256, 1024
    N, H, W = 2, 16, 12
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
        assert _layout(prog) == (1 if folded else 0), f"{case}: stream layout {_layout(prog)}"
        run_program(prog)
        got = view_to_nchw(y)
        fin = torch.isfinite(want) & (want.abs() < 6.0e4)                  # (the 1e5 channel overflows fp16 on every path)
        yt = ActView(torch.zeros((N, H, W, C), dtype=dtype, device=dev), C, 0)
        prog_t = make_program()
        record_bottleneck(prog_t, c1, c2, c3, xv, yt, name, fold=False)
        run_program(prog_t)
        rel = lambda a: ((a - want).abs() / (1.0 + want.abs()))[fin]
        err, err_t = rel(got).max().item(), rel(view_to_nchw(yt)).max().item()
        print(f"{name} {case}: max relative err 16-pixel folded {err:.3e} / table form {err_t:.3e}; mean {rel(got).mean().item():.2e} / {rel(view_to_nchw(yt)).mean().item():.2e}")
        assert err <= 1.5 * err_t + 1e-3 and rel(got).mean().item() <= 1.5 * rel(view_to_nchw(yt)).mean().item() + 1e-5, f"{case}: folded {err:.3e} vs table {err_t:.3e}"
        if case == "shift_beyond_fp16":
            assert torch.isinf(got[:, 7]).all() and (got[:, 7] > 0).all()
