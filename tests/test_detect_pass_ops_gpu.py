"""The detector's clip-pass kernels on the GPU through the C ABI (csrc/detect_pass_ops.hip): ft_topk_desc_f32, ft_proposal_rois_fwd
and ft_detect_select_fwd against tests/detect_pass_ref.py.  Every result is fully determined (a unique integer sort key, fp32
expressions rounded one by one), so every comparison is np.array_equal on the bits."""
import numpy as np
import pytest
import torch

from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_OK
from flowtrack.pytorch_amd.detection import ops

import detect_pass_ref as P

pytestmark = pytest.mark.gpu
F32 = np.float32
POISON = 0x7FABCDEF                                    # a NaN pattern no kernel writes


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- ft_topk_desc_f32 -----------------------------------------------------------------------------------------------------
def _topk(lib, scores, k, tail=8):
    n = len(scores)
    d = _dev(scores, F32)
    order = torch.full((k + tail,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((k + tail,), POISON, dtype=torch.int32, device="cuda")
    assert lib.ft_topk_desc_f32(_ptr(d), n, k, _ptr(order), _ptr(out), None, None) == FT_OK
    torch.cuda.synchronize()
    order, out = order.cpu().numpy(), out.cpu().numpy()
    assert (order[k:] == -7).all() and (out[k:] == POISON).all(), "wrote past k"
    return out[:k].view(F32), order[:k]


def _check_topk(lib, scores, k):
    scores = np.ascontiguousarray(scores, dtype=F32)
    got_v, got_i = _topk(lib, scores, k)
    want_v, want_i = P.topk_ref(scores, k)
    assert np.array_equal(got_i, want_i), f"n={len(scores)} k={k}: first difference at {int(np.flatnonzero(got_i != want_i)[0])}"
    assert np.array_equal(_bits(got_v), _bits(want_v)) and np.array_equal(_bits(got_v), _bits(scores[got_i]))


def _half_neighbours(n, seed):
    """Scores that differ only in their lowest mantissa bits around 0.5: what the synthetic RPN heads give."""
    rng = np.random.default_rng(seed)
    return (np.uint32(0x3F000000) + rng.integers(-1, 2, n).astype(np.int64)).astype(np.uint32).view(F32)


TOPK_CASES = {
    "one": lambda: (np.array([0.25], dtype=F32), 1),
    "n5000_all": lambda: (np.random.default_rng(0).standard_normal(5000).astype(F32), 5000),
    "rpn_random": lambda: (np.random.default_rng(1).uniform(0, 1, 21546).astype(F32), 6000),
    "all_equal": lambda: (np.full(9000, 0.5, dtype=F32), 6000),
    "two_values_cut_in_ties": lambda: (np.where(np.random.default_rng(2).uniform(size=9000) < 0.3, F32(0.75), F32(0.25)).astype(F32), 6000),
    "low_bit_around_half": lambda: (_half_neighbours(21546, 3), 6000),
    "descending_ramp": lambda: (np.arange(7001, 0, -1).astype(F32), 3000),
    "ascending_ramp": lambda: (np.arange(7001).astype(F32), 3000),
    "largest": lambda: (np.random.default_rng(4).integers(0, 4096, 65536).astype(F32), 16384),
    "blob_1000x1000": lambda: (np.random.default_rng(5).integers(0, 512, 35721).astype(F32), 6000),
    "k_not_pow2_small": lambda: (np.random.default_rng(7).integers(0, 9, 700).astype(F32), 300),
    "k1500_of_3000": lambda: (np.random.default_rng(9).integers(0, 40, 3000).astype(F32), 1500),
    "k3000_of_8192": lambda: (np.random.default_rng(8).standard_normal(8192).astype(F32), 3000),
    "specials": lambda: (np.tile(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 1e-45, -1e-45, 0.5], dtype=F32), 37), 200),
}


@pytest.mark.parametrize("case", sorted(TOPK_CASES))
def test_topk(hip_lib, case):
    scores, k = TOPK_CASES[case]()
    _check_topk(hip_lib, scores, k)
    if case == "all_equal":
        assert np.array_equal(_topk(hip_lib, scores, k)[1], np.arange(k))
    if case == "two_values_cut_in_ties":
        assert (scores == F32(0.75)).sum() < k                  # the cut falls inside the run of 0.25s


def test_topk_wrapper_and_refusals(hip_lib):
    from flowtrack.pytorch_amd.detection import proposal
    s = np.random.default_rng(6).integers(0, 50, 3000).astype(F32)
    v, i = proposal.topk_desc(_dev(s), 700)
    tv, ti = _dev(s).sort(descending=True, stable=True)
    assert i.dtype == torch.int32 and torch.equal(i.long(), ti[:700]) and torch.equal(v, tv[:700])
    p = _dev(np.zeros(16, dtype=F32))
    f = hip_lib.ft_topk_desc_f32
    assert f(None, 0, 0, None, None, None, None) == FT_OK
    assert f(_ptr(p), 16, 17, _ptr(p), _ptr(p), None, None) == FT_ERR_UNSUPPORTED
    assert f(_ptr(p), 65537, 4, _ptr(p), _ptr(p), None, None) == FT_ERR_UNSUPPORTED
    assert f(_ptr(p), 16, -1, _ptr(p), _ptr(p), None, None) == FT_ERR_INVALID_ARG
    assert f(_ptr(p), 16, 4, None, _ptr(p), None, None) == FT_ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---- ft_proposal_rois_fwd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 300, 450])
def test_proposal_rois(hip_lib, count):
    rng = np.random.default_rng(count)
    m, rows = 500, 300
    boxes = rng.uniform(0, 900, (m, 4)).astype(F32)
    keep = np.full(m, -1, dtype=np.int32)
    keep[:count] = rng.permutation(m)[:count]
    d_rois = _dev(rng.uniform(1, 2, (rows + 2, 5)).astype(F32))          # stale contents; two guard rows behind the buffer
    guard = d_rois[rows:].clone()
    d_n = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    d_boxes, d_keep, d_count = _dev(boxes), _dev(keep), _dev(np.array([count], dtype=np.int32))
    st = hip_lib.ft_proposal_rois_fwd(_ptr(d_boxes), _ptr(d_keep), _ptr(d_count), m, rows, _ptr(d_rois), _ptr(d_n), None)
    assert st == FT_OK
    torch.cuda.synchronize()
    want, n = P.proposal_rois_ref(boxes, keep, count, rows)
    assert int(d_n.item()) == n == min(count, rows)
    assert np.array_equal(_bits(d_rois[:rows].cpu().numpy()), _bits(want)) and torch.equal(d_rois[rows:], guard)


def test_proposal_rois_bad_keep_entries_address_nothing(hip_lib):
    boxes = np.arange(40, dtype=F32).reshape(10, 4)
    keep = np.array([3, 10, -2, 9, 1 << 30, 0, 0, 0, 0, 0], dtype=np.int32)
    d_rois = _dev(np.ones((6, 5), dtype=F32))
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_boxes, d_keep, d_count = _dev(boxes), _dev(keep), _dev(np.array([5], dtype=np.int32))
    assert hip_lib.ft_proposal_rois_fwd(_ptr(d_boxes), _ptr(d_keep), _ptr(d_count), 10, 6, _ptr(d_rois), _ptr(d_n), None) == FT_OK
    torch.cuda.synchronize()
    want, n = P.proposal_rois_ref(boxes, keep, 5, 6)
    assert n == 5 and np.array_equal(d_rois.cpu().numpy(), want) and not want[[1, 2, 4, 5]].any()


# ---- ft_detect_select_fwd -------------------------------------------------------------------------------------------------
def _person_case(seed, R, K, M, person=1, spread=60.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, spread, (R + M, 2)).astype(F32)
    wh = rng.uniform(5, 40, (R + M, 2)).astype(F32)
    boxes = np.concatenate((xy, xy + wh), 1).astype(F32)
    scores = (rng.integers(1, 12, R + M) / F32(16)).astype(F32)            # duplicate scores within and across the two groups
    cls_prob = rng.uniform(0, 1, (R, K)).astype(F32)
    pred = rng.uniform(0, 90, (R, 4 * K)).astype(F32)
    cls_prob[:, person], pred[:, 4 * person:4 * person + 4] = scores[:R], boxes[:R]
    extra = np.concatenate((boxes[R:], scores[R:, None]), 1).astype(F32)
    return cls_prob, pred, extra


def _select(lib, cls_prob, pred, n_rois, person, extra, extra_count, min_score, thresh, max_keep, cap):
    R, K = cls_prob.shape
    M = 0 if extra is None else len(extra)
    d_dets = _dev(np.full((cap + 1, 5), 7.0, dtype=F32))                   # stale contents; one guard row
    d_cnt = torch.full((1,), -3, dtype=torch.int32, device="cuda")
    d_nr = _dev(np.array([n_rois], dtype=np.int32))
    d_ec = _dev(np.array([extra_count], dtype=np.int32)) if extra_count is not None else None
    d_cp, d_pb = _dev(cls_prob.reshape(-1)) if R else None, _dev(pred.reshape(-1)) if R else None
    d_ex = None if extra is None else _dev(extra if M else np.full((1, 5), 9.0, dtype=F32))      # M = 0 with a pointer: not read
    st = lib.ft_detect_select_fwd(_ptr(d_cp), _ptr(d_pb), R, _ptr(d_nr), K, person, _ptr(d_ex), M, _ptr(d_ec), min_score, thresh, max_keep,
                                  cap, _ptr(d_dets), _ptr(d_cnt), None)
    assert st == FT_OK
    torch.cuda.synchronize()
    out = d_dets.cpu().numpy()
    assert (out[cap] == 7.0).all(), "wrote past cap"
    return out[:cap], int(d_cnt.item())


def _check_select(lib, cls_prob, pred, n_rois, person, extra, extra_count, min_score, thresh, max_keep, cap):
    got, n = _select(lib, cls_prob, pred, n_rois, person, extra, extra_count, min_score, thresh, max_keep, cap)
    want, wn = P.select_ref(cls_prob, pred, n_rois, person, extra, extra_count, min_score, thresh, max_keep, cap)
    assert n == wn and np.array_equal(_bits(got), _bits(want))
    return got, n


@pytest.mark.parametrize("n_rois", [0, 1, 300])
@pytest.mark.parametrize("extras", ["none", "all", "counted", "m0"])
def test_detect_select(hip_lib, n_rois, extras):
    M = {"none": 0, "all": 20, "counted": 20, "m0": 0}[extras]
    cls_prob, pred, extra = _person_case(10 + n_rois, 300, 3, M)
    ex = extra if extras in ("all", "counted") else (np.zeros((0, 5), dtype=F32) if extras == "m0" else None)
    ec = 9 if extras == "counted" else None
    got, n = _check_select(hip_lib, cls_prob, pred, n_rois, 1, ex, ec, 0.0, 0.3, 0, 300 + M)
    assert n >= min(1, n_rois + (M if ec is None else ec))
    # the existing GPU path on the concatenation detect_persons forms
    cat = np.concatenate((np.concatenate((pred[:n_rois, 4:8], cls_prob[:n_rois, 1:2]), 1), extra[:M if ec is None else ec]), 0).astype(F32)
    if len(cat):
        d = _dev(cat)
        assert np.array_equal(got[:n], d[ops.nms(d, 0.3)].cpu().numpy())


def test_detect_select_identical_and_disjoint_boxes(hip_lib):
    R, K = 200, 3
    cls_prob = np.random.default_rng(0).uniform(0.01, 1, (R, K)).astype(F32)
    pred = np.tile(np.array([10, 20, 50, 80], dtype=F32), (R, K))
    got, n = _check_select(hip_lib, cls_prob, pred, R, 2, None, None, 0.0, 0.3, 0, R)
    assert n == 1 and got[0, 4] == cls_prob[:, 2].max()                    # all identical: one survives
    x0 = (np.arange(R, dtype=F32) * 50)[:, None]
    pred = np.tile(np.concatenate((x0, np.zeros_like(x0), x0 + 30, np.full_like(x0, 30)), 1), (1, K)).astype(F32)
    got, n = _check_select(hip_lib, cls_prob, pred, R, 2, None, None, 0.0, 0.3, 0, R)
    assert n == R and np.array_equal(got[:, 4], np.sort(cls_prob[:, 2])[::-1])          # disjoint: all survive, by score


def test_detect_select_screen_and_caps(hip_lib):
    cls_prob, pred, extra = _person_case(77, 300, 3, 30, spread=600.0)
    full, n_full = _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 0.0, 0.3, 0, 330)
    assert n_full > 40
    got, n = _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 0.4, 0.3, 0, 330)
    assert 0 < n < n_full and (got[:n, 4] >= 0.4).all()
    assert _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 5.0, 0.3, 0, 330)[1] == 0      # everything screened
    got, n = _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 0.0, 0.3, 17, 330)
    assert n == 17 and np.array_equal(got[:17], full[:17])
    got, n = _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 0.0, 0.3, 0, 9)                # cap below the survivors
    assert n == 9 and np.array_equal(got, full[:9])
    got, n = _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 0.0, 0.3, 50, 9)               # max_keep above cap: cap
    assert n == 9


def test_detect_select_at_the_limit_and_refusals(hip_lib):
    cls_prob, pred, extra = _person_case(5, 300, 3, 724, spread=2000.0)
    got, n = _check_select(hip_lib, cls_prob, pred, 300, 1, extra, None, 0.0, 0.3, 0, 1024)
    assert n > 300
    p = _dev(np.zeros(4096 * 12, dtype=F32))
    c = torch.zeros(1, dtype=torch.int32, device="cuda")
    f = hip_lib.ft_detect_select_fwd
    assert f(_ptr(p), _ptr(p), 300, _ptr(c), 3, 1, _ptr(p), 725, None, 0.0, 0.3, 0, 1025, _ptr(p), _ptr(c), None) == FT_ERR_UNSUPPORTED
    assert f(_ptr(p), _ptr(p), 300, _ptr(c), 3, 3, None, 0, None, 0.0, 0.3, 0, 300, _ptr(p), _ptr(c), None) == FT_ERR_INVALID_ARG
    assert f(_ptr(p), _ptr(p), 300, _ptr(c), 3, -1, None, 0, None, 0.0, 0.3, 0, 300, _ptr(p), _ptr(c), None) == FT_ERR_INVALID_ARG
    assert f(_ptr(p), _ptr(p), 300, _ptr(c), 3, 1, None, 0, None, 0.0, 0.3, 0, 0, _ptr(p), _ptr(c), None) == FT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert int(c.item()) == 0 and not p.any()                             # the refused calls wrote nothing
