"""The HIP Correlation / Resample2d / ChannelNorm kernels against the REFERENCE'S OWN NUMBERS: tests/golden/flowops_golden.npz,
written by the reference's .cu kernels compiled for the CPU (tests/golden/make_flowops_golden.py).  Reads the committed fixture
only.  Forward: the NCHW entry point and every NHWC kernel form (asserted through ft_correlation_nhwc_form) at the bars those
kernels meet against the C oracle in test_flow_gpu.py (1e-5 fp32, 1e-3 fp16; ChannelNorm 1e-6; the fused warp stage its own
1e-5), bit for bit on the exact-data cases.  Backward: where the reference's backward is the gradient of its forward
(kernel_size 1, stride1 1; tests/test_flowops_pinned_cpu.py shows both in the fixture), within twice the derived rounding bound
of tests/flowops_pinned.py — kernel and fixture each obey it — and bit for bit on the exact-data cases.
Every output goes into a NaN-poisoned buffer between NaN guards."""
import ctypes

import numpy as np
import pytest
import torch

import correlation_cases as cc
import flowops_pinned as fp
from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd._lib import check

pytestmark = pytest.mark.gpu
GUARD = 256


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class Guarded:
    """`shape` elements of NaN between two NaN guards; done() returns the CPU copy after checking the guards."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.whole = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + self.n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def done(self, all_written=True):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.whole[:GUARD]).all()) and bool(torch.isnan(self.whole[GUARD + self.n:]).all()), "guard overwritten"
        out = self.t.cpu()
        if all_written:
            assert not bool(torch.isnan(out).any()), "elements left unwritten (or NaN written)"
        return out


def _report(what, got, want, tol):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
    print(f"{what}: max abs err {err:.3e} (bar {tol:.0e})")
    assert err <= tol, what


def _within2(what, got, want, bnd):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    ratio = fp.worst(err, 2.0 * np.asarray(bnd))
    print(f"{what}: max abs err {float(err.max()):.3e}, max err / (2 * bound) {ratio:.3f}")
    assert ratio <= 1.0, what


# ---- correlation forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(fp.N_CORR))
def test_correlation_nchw_matches_the_reference_kernels(hip_lib, i):
    c, (pad, k, md, s1, s2) = fp.corr(i)
    B, C, H, W = c["in1"].shape
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(hip_lib.ft_correlation_out_shape(C, H, W, pad, k, md, s1, s2, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow)))
    assert (B, oc.value, oh.value, ow.value) == c["out"].shape
    ga, gb, out = _cuda(c["in1"]), _cuda(c["in2"]), Guarded(c["out"].shape)
    check(hip_lib.ft_correlation_fwd(ga.data_ptr(), gb.data_ptr(), out.ptr(), B, C, H, W, pad, k, md, s1, s2, 1, _stream()))
    got = out.done().numpy()
    _report(f"corr{i} NCHW", got, c["out"], 1e-5)
    if i in fp.CORR_EXACT:
        assert np.array_equal(got, c["out"])


# fixture case, expected form, dtype, channel count the features are zero-padded to (nelems = that count: the result is scaled
# back by cpad / C, a power of two wherever bit equality is asked), y_cstride, y_coff, activation.  d 20 with ReLU is the only
# way into the one-row matrix-core kernel at FlowNetC's displacement; its fixture is max(want, 0).
NHWC_ROWS = [
    (0, cc.VALU, cc.F32, 8, 32, 3, cc.NONE),
    (1, cc.VALU, cc.F32, 40, 448, 4, cc.NONE),
    (4, cc.VALU, cc.F32, 8, 32, 3, cc.NONE),
    (2, cc.VALU, cc.F32, 64, 448, 4, cc.NONE),
    (2, cc.VALU, cc.F32, 256, 480, 32, cc.NONE),
    (2, cc.VALU, cc.F16, 64, 448, 4, cc.NONE),
    (2, cc.ROWS64, cc.F16, 256, 464, 8, cc.NONE),
    (2, cc.ROWS, cc.F16, 256, 445, 3, cc.NONE),
    (2, cc.MFMA, cc.F16, 256, 449, 3, cc.RELU),
    (5, cc.VALU, cc.F32, 8, 32, 3, cc.NONE),
    (5, cc.VALU, cc.F16, 8, 32, 3, cc.NONE),
    (5, cc.MFMA, cc.F16, 256, 33, 3, cc.NONE),
    (6, cc.VALU, cc.F32, 8, 448, 4, cc.NONE),
    (6, cc.VALU, cc.F16, 8, 448, 4, cc.NONE),
    (6, cc.ROWS64, cc.F16, 256, 464, 8, cc.NONE),
    (6, cc.ROWS, cc.F16, 256, 445, 3, cc.NONE),
    (6, cc.MFMA, cc.F16, 256, 449, 3, cc.RELU),
]


@pytest.mark.parametrize("row", NHWC_ROWS, ids=lambda r: f"corr{r[0]}-{cc.FORM_NAMES[r[1]]}-{'fp16' if r[2] == cc.F16 else 'fp32'}-c{r[3]}")
def test_correlation_nhwc_forms_match_the_reference_kernels(hip_lib, row):
    i, form, dtype, cpad, ycs, yco, act = row
    c, (pad, k, md, s1, s2) = fp.corr(i)
    B, C, H, W = c["in1"].shape
    assert k == 1 and s1 == 1 and pad == md and cpad >= C            # what the in-network kernels fix
    assert hip_lib.ft_correlation_nhwc_form(B, cpad, H, W, md, s2, cpad, ycs, yco, act, 0.0, dtype) == form
    tdt = torch.float16 if dtype == cc.F16 else torch.float32
    feats = []
    for a in (c["in1"], c["in2"]):
        f = torch.zeros((B, H, W, cpad), dtype=tdt, device="cuda")
        f[..., :C] = torch.from_numpy(a).permute(0, 2, 3, 1).to("cuda", tdt)
        if dtype == cc.F16 and (i == 2 or i in fp.CORR_EXACT):
            assert torch.equal(f[..., :C].float().cpu(), torch.from_numpy(a).permute(0, 2, 3, 1))    # fp16 holds these inputs exactly
        feats.append(f)
    y = Guarded((B, H, W, ycs), tdt)
    check(hip_lib.ft_correlation_nhwc_fwd(feats[0].data_ptr(), feats[1].data_ptr(), y.ptr(), B, cpad, H, W, md, s2, cpad, ycs, yco,
                                          act, 0.0, dtype, _stream()))
    out = y.done(all_written=False)
    dd = c["out"].shape[1]
    outside = torch.cat([out[..., :yco], out[..., yco + dd:]], -1)
    assert bool(torch.isnan(outside).all()), "channels outside [y_coff, y_coff + D*D) were written"
    got = out[..., yco:yco + dd].permute(0, 3, 1, 2).double().numpy() * (cpad / C)
    assert not np.isnan(got).any()
    want = np.maximum(c["out"], 0) if act == cc.RELU else c["out"]
    _report(f"corr{i} NHWC {cc.FORM_NAMES[form]}", got, want, 1e-3 if dtype == cc.F16 else 1e-5)
    if i in fp.CORR_EXACT:
        assert np.array_equal(got, want.astype(np.float64))


# ---- resample2d / channelnorm forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(fp.N_RS))
def test_resample2d_matches_the_reference_kernels(hip_lib, i):
    r = fp.rs(i)
    B, C, H, W = r["img"].shape
    gi, gf, out = _cuda(r["img"]), _cuda(r["flow"]), Guarded(r["out"].shape)
    check(hip_lib.ft_resample2d_fwd(gi.data_ptr(), gf.data_ptr(), out.ptr(), B, C, H, W, _stream()))
    got = out.done().numpy()
    _report(f"rs{i}", got, r["out"], 1e-5)
    if i == fp.RS_EXACT:
        assert np.array_equal(got, r["out"])


@pytest.mark.parametrize("i", range(fp.N_CN))
def test_channelnorm_matches_the_reference_kernels(hip_lib, i):
    n = fp.cn(i)
    B, C, H, W = n["x"].shape
    gx, out = _cuda(n["x"]), Guarded(n["out"].shape)
    check(hip_lib.ft_channelnorm_fwd(gx.data_ptr(), out.ptr(), B, C, H, W, _stream()))
    got = out.done().numpy()
    fin = np.isfinite(n["out"])
    assert np.array_equal(np.isposinf(got), ~fin), "the pixel whose squares overflow must come out +inf, and no other"
    assert (~fin).sum() == (1 if i == fp.CN_INF else 0)
    _report(f"cn{i}", got[fin], n["out"][fin], 1e-6)
    if i == fp.CN_INF:
        assert got[0, 0, 1, 2] == 0.0


@pytest.mark.parametrize("i", [0, fp.RS_EXACT])
def test_fused_warp_concat_matches_the_reference_kernels(hip_lib, i):
    """ft_flow_warp_concat = Resample2d + ChannelNorm + cat.  img1 and the flow are the fixture's Resample2d inputs, so channels
    6..8 must be the reference's Resample2d output; img0 = x + that output for rs0, x the ChannelNorm input of the same shape, so
    channel 11 = |img0 - warp| must be the reference's ChannelNorm output up to the two roundings of forming and undoing the sum
    and the kernel's own warp error, each a few 1e-7 per channel: well inside the fused kernel's 1e-5 bar (test_glue_gpu.py).
    On the exact map img0 = 0, the warp must be bit-equal, and the norm is compared with the float64 root of the exact squares."""
    r = fp.rs(i)
    B, C, H, W = r["img"].shape
    assert C == 3
    if i == 0:
        n = fp.cn(0)
        assert n["x"].shape == r["img"].shape
        img0 = (n["x"].astype(np.float64) + r["out"].astype(np.float64)).astype(np.float32)
    else:
        img0 = np.zeros_like(r["img"])
    xl, xp, yl, yp, div = 1, W + 3, 2, W + 5, 20.0
    x6 = torch.full((B, H, xp, 8), float("nan"), dtype=torch.float32, device="cuda")      # a tap read from a pad column shows
    x6[:, :, xl:xl + W, :3] = torch.from_numpy(img0).permute(0, 2, 3, 1).cuda()
    x6[:, :, xl:xl + W, 3:6] = torch.from_numpy(r["img"]).permute(0, 2, 3, 1).cuda()
    gf, y = _cuda(r["flow"]), Guarded((B, H, yp, 16))
    check(hip_lib.ft_flow_warp_concat(x6.data_ptr(), gf.data_ptr(), ctypes.c_float(div), y.ptr(), B, H, W, xl, xp, yl, yp, _lib.FT_F32,
                                      _stream()))
    out = y.done()
    live = out[:, :, yl:yl + W].permute(0, 3, 1, 2).numpy()
    assert not out[:, :, :yl].any() and not out[:, :, yl + W:].any() and not live[:, 12:].any()
    assert np.array_equal(live[:, 3:6], r["img"]) and np.array_equal(live[:, :3], img0)
    _report(f"rs{i} fused warp", live[:, 6:9], r["out"], 1e-5)
    _report(f"rs{i} fused flow / div_flow", live[:, 9:11], r["flow"].astype(np.float64) / div, 1e-5)
    if i == 0:
        _report("cn0 fused |img0 - warp|", live[:, 11:12], fp.cn(0)["out"], 1e-5)
    else:
        assert np.array_equal(live[:, 6:9], r["out"])
        want = np.sqrt((r["out"].astype(np.float64) ** 2).sum(1, keepdims=True))                # integers and quarters: exact squares
        _report("rs exact fused |0 - warp|", live[:, 11:12], want, 1e-5)


# ---- backward --------------------------------------------------------------------------------------------------------------
ADJOINT_CORR = [i for i in range(fp.N_CORR) if fp.corr_is_adjoint_case(fp.corr(i)[1])]


def test_backward_cases_are_the_ones_where_the_adjoint_is_the_reference():
    assert ADJOINT_CORR == [0, 1, 2, 4, 5, 6]


@pytest.mark.parametrize("i", ADJOINT_CORR)
def test_correlation_backward_matches_the_reference_kernels(hip_lib, i):
    c, p = fp.corr(i)
    B, C, H, W = c["in1"].shape
    _, _, b1, b2 = fp.corr_bwd_loops(i)
    ga, gb, gg = _cuda(c["in1"]), _cuda(c["in2"]), _cuda(c["gout"])
    o1, o2 = Guarded(c["in1"].shape), Guarded(c["in2"].shape)
    check(hip_lib.ft_correlation_bwd(ga.data_ptr(), gb.data_ptr(), gg.data_ptr(), o1.ptr(), o2.ptr(), B, C, H, W, *p, 1, _stream()))
    g1, g2 = o1.done().numpy(), o2.done().numpy()
    _within2(f"corr{i} grad_in1", g1, c["gin1"], b1)
    _within2(f"corr{i} grad_in2", g2, c["gin2"], b2)
    if i in fp.CORR_EXACT:
        assert np.array_equal(g1 + np.float32(0), c["gin1"] + np.float32(0)) and np.array_equal(g2 + np.float32(0), c["gin2"] + np.float32(0))


@pytest.mark.parametrize("i", range(fp.N_RS))
def test_resample2d_backward_matches_the_reference_kernels(hip_lib, i):
    """The reference's image gradient equals the adjoint on every element, also where negative coordinates scatter (both
    neighbours clamp to index 0, see test_flowops_pinned_cpu.py), so nothing is masked out."""
    r = fp.rs(i)
    B, C, H, W = r["img"].shape
    bi, bf, _ = fp.rs_bwd_bounds(r)
    gi, gf, gg = _cuda(r["img"]), _cuda(r["flow"]), _cuda(r["gout"])
    o1, o2 = Guarded(r["img"].shape), Guarded(r["flow"].shape)
    check(hip_lib.ft_resample2d_bwd(gi.data_ptr(), gf.data_ptr(), gg.data_ptr(), o1.ptr(), o2.ptr(), B, C, H, W, _stream()))
    g1, g2 = o1.done().numpy(), o2.done().numpy()
    _within2(f"rs{i} grad_in1", g1, r["gimg"], bi)
    _within2(f"rs{i} grad_flow", g2, r["gflow"], bf)
    if i == fp.RS_EXACT:
        assert np.array_equal(g1 + np.float32(0), r["gimg"] + np.float32(0)) and np.array_equal(g2 + np.float32(0), r["gflow"] + np.float32(0))


@pytest.mark.parametrize("i", range(fp.N_CN))
def test_channelnorm_backward_matches_the_reference_kernels(hip_lib, i):
    n = fp.cn(i)
    B, C, H, W = n["x"].shape
    _, bnd = fp.cn_bwd(n)
    gx, go, gg, out = _cuda(n["x"]), _cuda(n["out"]), _cuda(n["gout"]), Guarded(n["x"].shape)
    check(hip_lib.ft_channelnorm_bwd(gx.data_ptr(), go.data_ptr(), gg.data_ptr(), out.ptr(), B, C, H, W, _stream()))
    got = out.done().numpy()
    _within2(f"cn{i} grad_in1", got, n["gx"], bnd)
    if i == fp.CN_INF:
        assert not got[0, :, 1, 2].any() and not got[0, :, 2, 3].any()
