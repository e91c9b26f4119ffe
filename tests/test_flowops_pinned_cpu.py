"""Correlation / Resample2d / ChannelNorm pinned to the reference's own kernels, host side.

tests/golden/flowops_golden.npz holds what the reference's .cu kernels computed (compiled for the CPU, oracle/cuda_on_cpu/).
Against it: the C oracle bit for bit, the numpy / float64 formulations and the restated backward loops within the derived
rounding bound of tests/flowops_pinned.py (bit for bit on the exact-data cases), and the two documented departures of the
reference's backward from the gradient of its forward.  The live-library tests run only where oracle/_ref/ was built (the
reference checkout is present); the fixture tests never skip.  No GPU needed."""
import numpy as np
import pytest
import torch

import flow_grad_ref as ref
import flowops_pinned as fp
from oracle import ops_ref, ref_ops

CORR = list(range(fp.N_CORR))
RS = list(range(fp.N_RS))
CN = list(range(fp.N_CN))
live = pytest.mark.skipif(not ref_ops.available(), reason="oracle/_ref/ not built: no reference checkout on this machine")


def _within(got, want, bnd, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    ratio = fp.worst(err, bnd)
    print(f"{what}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert ratio <= 1.0, what


def test_fixture_holds_every_case_and_the_launch_counts():
    assert (fp.N_CORR, fp.N_RS, fp.N_CN) == (7, 3, 3)
    assert fp.G["launch_counts"].tolist() == [7, 3, 2]
    want = [(2, 5, 6, 7, 4, 1, 4, 1, 2), (1, 33, 5, 5, 20, 1, 20, 1, 2), (1, 64, 6, 8, 20, 1, 20, 1, 2), (1, 40, 8, 9, 3, 3, 2, 2, 1),
            (1, 6, 9, 13, 6, 1, 6, 1, 3), (1, 8, 6, 7, 4, 1, 4, 1, 2), (1, 8, 6, 8, 20, 1, 20, 1, 2)]
    for i, case in enumerate(want):
        c, p = fp.corr(i)
        assert c["in1"].shape + p == case
    for i in fp.CORR_EXACT:
        c, _ = fp.corr(i)
        for k in ("in1", "in2", "gout"):
            assert np.array_equal(c[k], np.round(c[k])) and np.abs(c[k]).max() <= 3
    assert [fp.rs(i)["img"].shape for i in RS] == [(2, 3, 9, 11), (1, 5, 24, 23), (1, 3, 8, 10)]
    assert [fp.cn(i)["x"].shape for i in CN] == [(2, 3, 9, 11), (1, 1, 5, 7), (1, 2, 4, 6)]
    r = fp.rs(fp.RS_EXACT)
    _, _, H, W = r["img"].shape
    xf, yf, fx, fy, _ = fp.rs_geometry(r["flow"], H, W)
    assert np.array_equal(r["flow"] * 4, np.round(r["flow"] * 4)) and np.array_equal(r["img"], np.round(r["img"]))
    assert (xf < 0).any() and (yf < 0).any() and fp.rs_negative_sources(r).any()
    assert ((xf == fx) & (yf == fy) & (xf >= 0) & (xf < W) & (yf >= 0) & (yf < H)).any()
    assert ((xf == W - 1) & (yf == H - 1)).any()
    for i in RS:
        r = fp.rs(i)
        xf, yf, *_ = fp.rs_geometry(r["flow"], *r["img"].shape[2:])
        assert max(np.abs(xf).max(), np.abs(yf).max()) < 2.0 ** 31
    _, _, fx, _, idx = fp.rs_geometry(fp.rs(1)["flow"], 24, 23)
    assert float(np.mean(fx != idx["xL"])) > 0.5         # rs1: most samples clamp
    n = fp.cn(fp.CN_INF)
    assert np.isinf(n["out"][0, 0, 2, 3]) and n["out"][0, 0, 1, 2] == 0 and not n["x"][0, :, 1, 2].any()


# ---- forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CORR)
def test_correlation_c_oracle_is_bit_equal(oracle_lib, i):
    c, p = fp.corr(i)
    assert np.array_equal(ops_ref.correlation_c(c["in1"], c["in2"], *p), c["out"])


@pytest.mark.parametrize("i", CORR)
def test_correlation_formulations_within_bound(i):
    c, p = fp.corr(i)
    bnd = fp.corr_fwd_bound(c, p)
    _within(ops_ref.correlation_np(c["in1"], c["in2"], *p), c["out"], bnd, f"corr{i} correlation_np")
    with torch.no_grad():
        f64 = ref.correlation_fwd(torch.from_numpy(c["in1"]).double(), torch.from_numpy(c["in2"]).double(), *p).numpy()
    _within(f64, c["out"], bnd, f"corr{i} flow_grad_ref.correlation_fwd")
    if i in fp.CORR_EXACT:
        assert np.array_equal(f64, c["out"])


@pytest.mark.parametrize("i", RS)
def test_resample2d_forward(oracle_lib, i):
    r = fp.rs(i)
    assert np.array_equal(ops_ref.resample2d_c(r["img"], r["flow"]), r["out"])
    bnd = fp.rs_fwd_bound(r)
    _within(ops_ref.resample2d_np(r["img"], r["flow"]), r["out"], bnd, f"rs{i} resample2d_np")
    with torch.no_grad():
        f64 = ref.resample2d_fwd(torch.from_numpy(r["img"]).double(), torch.from_numpy(r["flow"]).double()).numpy()
    _within(f64, r["out"], bnd, f"rs{i} flow_grad_ref.resample2d_fwd")
    if i == fp.RS_EXACT:
        assert np.array_equal(f64, r["out"])


@pytest.mark.parametrize("i", CN)
def test_channelnorm_forward(oracle_lib, i):
    n = fp.cn(i)
    with np.errstate(over="ignore"):
        c_out = ops_ref.channelnorm_c(n["x"])
        np_out = ops_ref.channelnorm_np(n["x"])
        f64 = ref.channelnorm_fwd(torch.from_numpy(n["x"]).double()).numpy()
    assert np.array_equal(c_out, n["out"])
    fin = np.isfinite(n["out"])
    assert np.isfinite(np_out[~fin]).all()              # the float64 sum holds 9e38 and its root is 3e19: only fp32 overflows
    bnd = fp.cn_fwd_bound(n)
    _within(np_out[fin], n["out"][fin], bnd[fin], f"cn{i} channelnorm_np")
    _within(f64[fin], n["out"][fin], bnd[fin], f"cn{i} flow_grad_ref.channelnorm_fwd")
    assert (~fin).sum() == (1 if i == fp.CN_INF else 0)


# ---- backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CORR)
def test_correlation_backward_loops_within_bound(i):
    """The restated loops write the input pixels (yi * stride1, xi * stride1) that lie inside the map.  For stride1 > 1 the
    reference's blocks with yi * stride1 >= H or xi * stride1 >= W write too, through the flat index, into the next row, the
    next channel or past the tensor (correlation_cuda_kernel.cu:194, :286): corr3 shows those writes, on no other element."""
    c, p = fp.corr(i)
    g1, g2, b1, b2 = fp.corr_bwd_loops(i)
    on = fp.corr_lattice(c["in1"].shape, p[3])
    _within(g1[on], c["gin1"][on], b1[on], f"corr{i} gradInput1")
    _within(g2[on], c["gin2"][on], b2[on], f"corr{i} gradInput2")
    if i in fp.CORR_EXACT:
        assert np.array_equal(g1.astype(np.float32), c["gin1"]) and np.array_equal(g2.astype(np.float32), c["gin2"])
    if p[3] == 1:
        assert on.all()
        return
    stray = fp.corr_stray_targets(c["in1"].shape, p[3])
    assert not c["gin1"][~on].any()                      # input1's blocks return before they write (xmin >= outputWidth)
    off2 = (c["gin2"] != 0) & ~on
    print(f"corr{i}: {int(off2.sum())} non-zero gradInput2 elements off the stride-{p[3]} lattice, all reachable by a stray write")
    assert off2.any() and not (off2 & ~stray).any()


@pytest.mark.parametrize("i", RS)
def test_resample2d_backward_loops_within_bound(i):
    r = fp.rs(i)
    gi, gf = ref.resample2d_bwd_loops(r["img"], r["flow"], r["gout"])
    bi, bf, _ = fp.rs_bwd_bounds(r)
    _within(gi, r["gimg"], bi, f"rs{i} gradInput1")
    _within(gf, r["gflow"], bf, f"rs{i} gradInput2")
    if i == fp.RS_EXACT:                                 # exact terms: the order of the atomic adds cannot matter
        assert np.array_equal(gi.astype(np.float32), r["gimg"]) and np.array_equal(gf.astype(np.float32), r["gflow"])


@pytest.mark.parametrize("i", CN)
def test_channelnorm_backward_within_bound(i):
    n = fp.cn(i)
    want, bnd = fp.cn_bwd(n)
    assert np.isfinite(n["gx"]).all()
    _within(want, n["gx"], bnd, f"cn{i} gradInput1")
    if i == fp.CN_INF:
        assert not n["gx"][0, :, 1, 2].any() and not n["gx"][0, :, 2, 3].any()      # 0 / 1e-9 and x / inf


# ---- the reference's backward against the gradient of its forward ----------------------------------------------------------------
@pytest.mark.parametrize("i", CORR)
def test_correlation_adjoint_against_the_reference_kernels(i):
    """Kernel 1, stride1 1: the adjoint is the reference.  corr3 (k = 3, stride1 = 2) shows the documented departure in the
    reference's own numbers: gradInput1 sums the output window [p-krad-md, p+krad-md] where the forward read [p-2krad-md, p-md]."""
    c, p = fp.corr(i)
    a1, a2 = fp.corr_adjoint(i)
    _, _, b1, b2 = fp.corr_bwd_loops(i)
    if fp.corr_is_adjoint_case(p):
        _within(a1, c["gin1"], b1, f"corr{i} adjoint vs gradInput1")
        _within(a2, c["gin2"], b2, f"corr{i} adjoint vs gradInput2")
    else:
        assert p[1] == 3
        on = fp.corr_lattice(a1.shape, p[3])             # the pixels the reference's blocks visit: off them it leaves zeros
        dep = np.abs(a1 - c["gin1"])[on].max() / np.abs(a1).max()
        print(f"corr{i}: max |adjoint - reference gradInput1| / max |adjoint| on the visited pixels = {dep:.3f}")
        assert dep > 1e-2


@pytest.mark.parametrize("i", RS)
def test_resample2d_adjoint_against_the_reference_kernels(i):
    """Resample2d's backward takes alpha = xf - int(xf) where its forward takes xf - floor(xf); the two differ at negative
    non-integer coordinates (alpha - 1 instead of alpha).  In the reference's own numbers the departure does NOT reach the
    gradient: at such a coordinate both neighbours clamp to column (row) 0, so the image gradient receives
    (1 - alpha) g + alpha g = g under either definition, and the flow gradient uses floor throughout.  So the adjoint equals the
    reference everywhere, within the rounding bound (whose sum |term| does see the weights 1 - alpha > 1 and alpha < 0), and bit
    for bit on the exact map."""
    r = fp.rs(i)
    _, _, H, W = r["img"].shape
    xf, yf, fx, fy, idx = fp.rs_geometry(r["flow"], H, W)
    neg = fp.rs_negative_sources(r)
    assert neg.any()
    nx, ny = (xf < 0) & (xf != fx), (yf < 0) & (yf != fy)
    assert (idx["xL"][nx] == 0).all() and (idx["xR"][nx] == 0).all() and (idx["yT"][ny] == 0).all() and (idx["yB"][ny] == 0).all()
    ai, af = fp.rs_adjoint(r)
    bi, bf, touched = fp.rs_bwd_bounds(r)
    assert touched.any() and not touched.all()
    _within(af, r["gflow"], bf, f"rs{i} adjoint vs gradInput2")
    _within(ai[~touched], r["gimg"][~touched], bi[~touched], f"rs{i} adjoint vs gradInput1 away from negative coordinates")
    _within(ai[touched], r["gimg"][touched], bi[touched], f"rs{i} adjoint vs gradInput1 where negative coordinates scatter")
    if i == fp.RS_EXACT:
        assert np.array_equal(ai.astype(np.float32), r["gimg"]) and np.array_equal(af.astype(np.float32), r["gflow"])


# ---- the live library ------------------------------------------------------------------------------------------------------
@live
def test_live_library_reproduces_the_fixture():
    for i in CORR:
        c, p = fp.corr(i)
        assert np.array_equal(ref_ops.correlation_fwd(c["in1"], c["in2"], *p), c["out"]), i
        g1, g2 = ref_ops.correlation_bwd(c["in1"], c["in2"], c["gout"], *p)
        assert np.array_equal(g1, c["gin1"]) and np.array_equal(g2, c["gin2"]), i
    for i in RS:
        r = fp.rs(i)
        assert np.array_equal(ref_ops.resample2d_fwd(r["img"], r["flow"]), r["out"]), i
        gi, gf = ref_ops.resample2d_bwd(r["img"], r["flow"], r["gout"])
        assert np.array_equal(gi, r["gimg"]) and np.array_equal(gf, r["gflow"]), i
    for i in CN:
        n = fp.cn(i)
        with np.errstate(over="ignore"):
            assert np.array_equal(ref_ops.channelnorm_fwd(n["x"]), n["out"]), i
            assert np.array_equal(ref_ops.channelnorm_bwd(n["x"], n["out"], n["gout"]), n["gx"]), i


def _sweep_corr_cases():
    """CORR_CASES of test_flow_gpu.py and test_flow_grad_gpu.py that the one-thread-at-a-time shim finishes in a few seconds:
    it switches fibers 2 * 32 * (D*D + 1) times per output pixel."""
    import test_flow_gpu
    import test_flow_grad_gpu
    out = []
    for case in test_flow_gpu.CORR_CASES + test_flow_grad_gpu.CORR_CASES:
        B, C, H, W, pad, k, md, s1, s2 = case
        oc, oh, ow = ref_ops.correlation_out_shape(C, H, W, pad, k, md, s1, s2)
        if case not in out and 64 * B * oh * ow * (oc + 1) <= 8e6:
            out.append(case)
    return out


@live
def test_live_library_equals_the_c_oracle_on_a_wider_sweep(oracle_lib):
    import test_flow_grad_gpu
    from flowtrack.pytorch_amd import synth
    cases = _sweep_corr_cases()
    assert len(cases) >= 8
    for case in cases:
        B, C, H, W, *p = case
        a = synth.normal(31, f"sa{case}", (B, C, H, W)).numpy()
        b = synth.normal(31, f"sb{case}", (B, C, H, W)).numpy()
        assert np.array_equal(ref_ops.correlation_fwd(a, b, *p), ops_ref.correlation_c(a, b, *p)), case
    n = 0
    for (B, C, H, W, kind) in test_flow_grad_gpu.RS_CASES:
        if kind not in ("noise", "far"):
            continue
        img = synth.normal(32, f"si{B}{C}{H}{W}", (B, C, H, W)).numpy()
        flow = test_flow_grad_gpu._flows(kind, B, H, W, f"sweep{B}{C}{H}{W}").numpy()
        assert np.array_equal(ref_ops.resample2d_fwd(img, flow), ops_ref.resample2d_c(img, flow)), (B, C, H, W, kind)
        assert np.array_equal(ref_ops.channelnorm_fwd(img), ops_ref.channelnorm_c(img)), (B, C, H, W)
        n += 1
    assert n == 4


@pytest.mark.skipif(not ref_ops.fma_available(), reason="no FMA build of oracle/_ref/ (no reference checkout, or a CPU without FMA)")
def test_contraction_changes_the_reference_by_less_than_the_bound():
    """nvcc contracts a * b + c into one FMA by default; the pinned library is built without contraction.  What contraction can
    change is bounded by the same rounding bound; the largest observed difference is printed (recorded in DESIGN.md)."""
    seen = {}

    def note(what, fused, plain, bnd):
        err = np.abs(fused.astype(np.float64) - plain.astype(np.float64))
        seen[what] = max(seen.get(what, 0.0), float(err.max()))
        assert fp.worst(err, bnd) <= 1.0, what

    for i in CORR:
        c, p = fp.corr(i)
        note("correlation forward", ref_ops.correlation_fwd(c["in1"], c["in2"], *p, fma=True), c["out"], fp.corr_fwd_bound(c, p))
        g1, g2 = ref_ops.correlation_bwd(c["in1"], c["in2"], c["gout"], *p, fma=True)
        _, _, b1, b2 = fp.corr_bwd_loops(i)
        on = fp.corr_lattice(c["in1"].shape, p[3])       # stride1 > 1: the stray writes off the lattice have no restated bound
        note("correlation backward", g1[on], c["gin1"][on], b1[on])
        note("correlation backward", g2[on], c["gin2"][on], b2[on])
    for i in RS:
        r = fp.rs(i)
        bi, bf, _ = fp.rs_bwd_bounds(r)
        note("resample2d forward", ref_ops.resample2d_fwd(r["img"], r["flow"], fma=True), r["out"], fp.rs_fwd_bound(r))
        gi, gf = ref_ops.resample2d_bwd(r["img"], r["flow"], r["gout"], fma=True)
        note("resample2d backward", gi, r["gimg"], bi)
        note("resample2d backward", gf, r["gflow"], bf)
    for i in CN:
        n = fp.cn(i)
        fin = np.isfinite(n["out"])
        with np.errstate(over="ignore"):
            out = ref_ops.channelnorm_fwd(n["x"], fma=True)
            gx = ref_ops.channelnorm_bwd(n["x"], n["out"], n["gout"], fma=True)
        assert np.array_equal(np.isfinite(out), fin)
        note("channelnorm forward", out[fin], n["out"][fin], fp.cn_fwd_bound(n)[fin])
        note("channelnorm backward", gx, n["gx"], fp.cn_bwd(n)[1])
    for what, v in seen.items():
        print(f"contraction on vs off, {what}: max abs difference {v:.3e}")
