"""CPU suite for the in-network correlation's four kernel forms: which form every row of tests/correlation_cases.py reaches
(ft_correlation_nhwc_form: host code, no device), the float64 reference (tests/correlation_ref.py) pinned to the C oracle and the
hand-derived impulse responses, and a float32 evaluation of the same sums held to the bound the GPU tests use."""
import os

import numpy as np
import pytest
import torch

import correlation_cases as cc
from conftest import GOLDEN
from correlation_ref import activation, correlation_nhwc_ref, error_bound, worst_ratio
from oracle import ops_ref

LEAKY_01 = (cc.LEAKY, 0.1)


def _form(lib, c, act=cc.LEAKY, slope=0.1, **kw):
    c = c._replace(**kw)
    return lib.ft_correlation_nhwc_form(c.B, c.C, c.H, c.W, c.d, c.s2, c.f_cstride, c.y_cstride, c.y_coff, act, slope, c.dtype)


def test_table_is_well_formed():
    names = [c.name for c in cc.CASES + cc.REFUSED + cc.INVALID]
    assert len(names) == len(set(names))
    assert {c.form for c in cc.CASES} == {cc.VALU, cc.MFMA, cc.ROWS, cc.ROWS64}
    for c in cc.CASES:
        assert c.B * c.H * c.W <= 4096, c.name                      # single launches on maps of a few thousand pixels


@pytest.mark.parametrize("case", cc.CASES + cc.REFUSED + cc.INVALID, ids=lambda c: c.name)
def test_every_row_reaches_its_form(hip_lib, case):
    assert _form(hip_lib, case, cc.NONE, 0.0) == case.form
    assert _form(hip_lib, case, *LEAKY_01) == case.form
    assert _form(hip_lib, case, cc.LEAKY, 2.0 ** -149) == case.form
    assert _form(hip_lib, case, cc.LEAKY, 1.0) == case.form
    for act, slope in ((cc.RELU, 0.0), (cc.LEAKY, 0.0), (cc.LEAKY, 1.5), (cc.LEAKY, -0.25), (cc.LEAKY, float("nan"))):
        want = cc.expected_form(case, act, slope)
        assert _form(hip_lib, case, act, slope) == want, (act, slope)


def test_form_boundaries(hip_lib):
    net = cc.Case("flownetc", cc.ROWS64, cc.F16, 16, 256, 48, 64, 20, 2, 256, 480, 32)     # FlowNetC at 512 x 384
    f = lambda **kw: _form(hip_lib, net, **kw)
    assert f() == cc.ROWS64
    assert (f(W=64), f(W=65)) == (cc.ROWS64, cc.ROWS)
    assert (f(d=20), f(d=18), f(d=22, y_cstride=568)) == (cc.ROWS64, cc.MFMA, cc.MFMA)
    assert (f(y_coff=32), f(y_coff=33), f(y_coff=36)) == (cc.ROWS64, cc.ROWS, cc.ROWS)
    assert (f(y_cstride=480), f(y_cstride=484)) == (cc.ROWS64, cc.ROWS)
    assert (f(C=256), f(C=264, f_cstride=264), f(C=248)) == (cc.ROWS64, cc.VALU, cc.VALU)
    assert (f(dtype=cc.F16), f(dtype=cc.F32, B=1, H=5, W=17)) == (cc.ROWS64, cc.VALU)
    assert (f(s2=2), f(s2=1, d=4, y_cstride=128), f(s2=4)) == (cc.ROWS64, cc.VALU, cc.VALU)
    assert (f(d=32, y_cstride=1096, y_coff=0), f(d=0), f(d=19), f(d=21)) == (cc.MFMA, cc.MFMA, cc.VALU, cc.VALU)
    assert f(f_cstride=288) == cc.ROWS64
    # 2 GiB of features: 32-bit buffer offsets end, the VALU form's size_t addressing takes over; 2 GiB of output: the one-row form's
    assert (f(B=728), f(B=729)) == (cc.ROWS64, cc.MFMA)              # B * 48 * 64 * 480 * 2 bytes of output
    assert (f(B=1365), f(B=1366)) == (cc.MFMA, cc.VALU)              # B * 48 * 64 * 256 * 2 bytes of features
    # the activation domain of the two rows forms: none, and leaky with a slope in (0, 1]; everything else runs the one-row form
    for kw in ({}, {"W": 65}):
        rows = cc.ROWS if kw else cc.ROWS64
        assert f(act=cc.NONE, **kw) == rows
        assert f(act=cc.LEAKY, slope=0.1, **kw) == rows
        assert f(act=cc.RELU, **kw) == cc.MFMA
        assert f(act=cc.LEAKY, slope=1.0, **kw) == rows
        assert f(act=cc.LEAKY, slope=0.0, **kw) == cc.MFMA
        assert f(act=cc.LEAKY, slope=1.5, **kw) == cc.MFMA
        assert f(act=cc.LEAKY, slope=-0.25, **kw) == cc.MFMA
    assert f(act=cc.RELU, C=64, f_cstride=64) == cc.VALU
    # refusals
    assert f(dtype=2) == -1 and f(B=0) == -1 and f(W=0) == -1 and f(d=-2) == -1 and f(s2=0) == -1
    assert f(f_cstride=260) == -1 and f(y_coff=-8) == -1 and f(y_coff=40) == -1


@pytest.mark.parametrize("name", ["valu16_c64_d5_s2_2x2x33_f64", "rows64_2x5x3_f288"])
def test_reference_matches_the_c_oracle(oracle_lib, name):
    c = cc.by_name(name)
    f1, f2 = cc.make_features(c)
    want, S = correlation_nhwc_ref(f1, f2, c.C, c.d, c.s2, cc.NONE, 0.0)
    a = f1[..., :c.C].float().permute(0, 3, 1, 2).contiguous().numpy()
    b = f2[..., :c.C].float().permute(0, 3, 1, 2).contiguous().numpy()
    oracle = ops_ref.correlation_c(a, b, c.d, 1, c.d, 1, c.s2).transpose(0, 2, 3, 1)
    assert oracle.shape == tuple(want.shape)
    # the oracle accumulates in fp32 in its own order: the same bound, without the fp16 output terms
    bound = error_bound(want, S, c.C, False).numpy()
    assert (np.abs(oracle - want.numpy()) <= 2 * bound).all()
    lk, _ = correlation_nhwc_ref(f1, f2, c.C, c.d, c.s2, cc.LEAKY, 0.1)
    rl, _ = correlation_nhwc_ref(f1, f2, c.C, c.d, c.s2, cc.RELU, 0.0)
    assert torch.equal(lk, torch.where(want > 0, want, 0.1 * want)) and torch.equal(rl, want.clamp(min=0))
    assert (S >= want.abs()).all()


def test_reference_matches_the_impulse_known_answers():
    G = np.load(os.path.join(GOLDEN, "correlation_kat.npz"))
    seen = 0
    for n in sorted({k.split(".")[0] for k in G.files}):
        pad, k, d, s1, s2 = (int(v) for v in G[n + ".params"])
        if not (k == 1 and s1 == 1 and pad == d):
            continue
        a, b, out = (torch.from_numpy(G[n + s]) for s in (".in1", ".in2", ".out"))
        want, S = correlation_nhwc_ref(a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1), a.shape[1], d, s2, cc.NONE, 0.0)
        out = out.permute(0, 2, 3, 1).double()
        assert ((want - out).abs() <= 2.0 ** -23 * out.abs()).all(), n      # the stored answers are fp32
        assert (S >= want.abs()).all() and ((S > 0) == (out != 0)).all(), n
        seen += 1
    assert seen >= 2


def _float32_eval(c, f1, f2, act, slope):
    """The kernels' arithmetic in numpy: fp32 products summed one channel after the other, * fp32(1/C), activation, output rounding."""
    a = f1[..., :c.C].float().numpy()
    b = np.zeros((c.B, c.H + 2 * c.d, c.W + 2 * c.d, c.C), np.float32)
    b[:, c.d:c.d + c.H, c.d:c.d + c.W] = f2[..., :c.C].float().numpy()
    drad = c.d // c.s2
    cells = []
    for tj in range(-drad, drad + 1):
        for ti in range(-drad, drad + 1):
            y0, x0 = c.d + tj * c.s2, c.d + ti * c.s2
            prod = a * b[:, y0:y0 + c.H, x0:x0 + c.W]
            cells.append(np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1])
    v = np.stack(cells, -1) * np.float32(1.0 / c.C)
    k = np.float32(0.0 if act == cc.RELU else slope if act == cc.LEAKY else 1.0)
    v = np.where(v > 0, v, v * k).astype(np.float32)
    return v.astype(np.float16).astype(np.float64) if c.dtype == cc.F16 else v.astype(np.float64)


_UNIQUE = list({cc.data_key(c): c for c in cc.CASES}.values())


@pytest.mark.parametrize("c", _UNIQUE, ids=lambda c: c.name)
def test_float32_evaluation_stays_inside_the_bound(c):
    """The bound of the GPU tests is derived, not tuned: before any kernel is held to it, a plain sequential fp32 evaluation of
    every row's sums has to fit inside 1 x bound - the factor 2 the GPU tests add is for the MFMA's summation order alone
    (rows that share their feature values are evaluated once)."""
    f1, f2 = cc.make_features(c)
    raw, S = cc.reference(c)
    want = activation(raw, *LEAKY_01)
    got = _float32_eval(c, f1, f2, *LEAKY_01)
    assert np.isfinite(got).all()                                      # the NaN gap channels stay out
    ratio = worst_ratio((torch.from_numpy(got) - want).abs(), error_bound(want, S, c.C, c.dtype == cc.F16))
    print(f"{c.name}: fp32 evaluation err / bound = {ratio:.3f}")
    assert ratio <= 1.0
