"""The detector's clip pass without a GPU: tests/detect_pass_ref.py pinned to torch's stable descending sort and to detect_ref.nms on
the concatenation detect_persons forms, and the refusals of the three C entries (the library loads without a GPU; a refused call
launches nothing)."""
import ctypes

import numpy as np
import torch

from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_OK

import detect_pass_ref as P
import detect_ref

F32 = np.float32


def _torch_topk(scores, k):
    v, i = torch.from_numpy(scores).sort(descending=True, stable=True)
    return v[:k].numpy(), i[:k].numpy().astype(np.int32)


def special_scores():
    """Ties, both zeros, both infinities, NaNs of both signs and payloads, denormals, neighbours around 0.5."""
    nan2 = np.array([0xFFC00001], dtype=np.uint32).view(F32)[0]            # a negative NaN with a payload
    half = np.array([0x3F000000 + d for d in (-2, -1, 0, 1, 2)], dtype=np.uint32).view(F32)
    s = [0.0, -0.0, 1.0, np.nan, -1.0, np.inf, -np.inf, 0.0, -0.0, 1.0, nan2, 1e-45, -1e-45, np.inf, -np.inf, 3.5, 3.5, -2.25, -2.25]
    return np.concatenate((np.array(s, dtype=F32), half, half[::-1], np.array([np.nan, 0.5, -0.0], dtype=F32)))


def test_topk_ref_is_torchs_stable_descending_sort():
    rng = np.random.default_rng(3)
    cases = [special_scores(), rng.standard_normal(1000).astype(F32), rng.integers(0, 4, 500).astype(F32),
             np.full(300, 0.5, dtype=F32), np.arange(200, dtype=F32), -np.arange(200, dtype=F32)]
    for s in cases:
        for k in (1, len(s) // 2, len(s)):
            got_v, got_i = P.topk_ref(s, k)
            want_v, want_i = _torch_topk(s, k)
            assert np.array_equal(got_i, want_i), (len(s), k)
            assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(got_v.view(np.uint32), s[got_i].view(np.uint32))
    s = special_scores()
    _, order = P.topk_ref(s, len(s))
    nans = np.flatnonzero(np.isnan(s))
    assert order[:len(nans)].tolist() == nans.tolist()                     # NaN in front, in index order
    zeros = np.flatnonzero(s == 0)
    assert [i for i in order if s[i] == 0] == zeros.tolist()               # -0.0 ties with +0.0
    keys = P.order_key(s).astype(np.int64)
    assert len(np.unique(keys * 65536 + (65535 - np.arange(len(s))))) == len(s) and keys.min() >= 0x007FFFFF


def test_proposal_rois_ref():
    boxes = np.arange(24, dtype=F32).reshape(6, 4)
    keep = np.array([4, 0, 5, -1, -1, -1], dtype=np.int32)
    rois, n = P.proposal_rois_ref(boxes, keep, 3, 5)
    assert n == 3 and np.array_equal(rois[:3, 1:], boxes[[4, 0, 5]]) and not rois[3:].any() and not rois[:, 0].any()
    assert P.proposal_rois_ref(boxes, keep, 3, 2)[1] == 2 and P.proposal_rois_ref(boxes, keep, 0, 4)[1] == 0
    assert P.proposal_rois_ref(boxes, keep, 9, 8)[1] == 6                 # never more than the keep list holds


def _person_case(rng, R, K, M):
    xy = rng.uniform(0, 60, (R + M, 2)).astype(F32)
    wh = rng.uniform(5, 40, (R + M, 2)).astype(F32)
    boxes = np.concatenate((xy, xy + wh), 1).astype(F32)
    scores = (rng.integers(0, 12, R + M) / F32(16)).astype(F32)            # many duplicate scores, across both groups
    cls_prob = rng.uniform(0, 1, (R, K)).astype(F32)
    pred = rng.uniform(0, 90, (R, 4 * K)).astype(F32)
    cls_prob[:, 1], pred[:, 4:8] = scores[:R], boxes[:R]
    extra = np.concatenate((boxes[R:], scores[R:, None]), 1).astype(F32)
    return cls_prob, pred, extra


def test_select_ref_is_detect_persons_nms():
    rng = np.random.default_rng(5)
    for R, M in ((40, 0), (40, 7), (1, 3), (0, 5)):
        cls_prob, pred, extra = _person_case(rng, R, 3, M)
        cat = np.concatenate((np.concatenate((pred[:, 4:8], cls_prob[:, 1:2]), 1), extra), 0)      # what detect_persons forms
        want = cat[detect_ref.nms(cat, 0.3)]
        cap = R + M
        dets, cnt = P.select_ref(cls_prob, pred, R, 1, extra if M else None, None, 0.0, 0.3, 0, cap)
        assert cnt == len(want) and np.array_equal(dets[:cnt], want) and not dets[cnt:].any()
        assert 0 < cnt <= cap
    cls_prob, pred, extra = _person_case(rng, 40, 3, 7)
    full, n_full = P.select_ref(cls_prob, pred, 40, 1, extra, None, 0.0, 0.3, 0, 47)
    dets, cnt = P.select_ref(cls_prob, pred, 40, 1, extra, None, 0.0, 0.3, 3, 47)
    assert cnt == 3 and np.array_equal(dets[:3], full[:3])                                         # max_keep: the first survivors
    dets, cnt = P.select_ref(cls_prob, pred, 40, 1, extra, None, 0.5, 0.3, 0, 47)
    assert 0 < cnt < n_full and (dets[:cnt, 4] >= 0.5).all()
    assert P.select_ref(cls_prob, pred, 40, 1, extra, None, 2.0, 0.3, 0, 47)[1] == 0
    part, n_part = P.select_ref(cls_prob, pred, 10, 1, extra, 2, 0.0, 0.3, 0, 47)                    # device counts cut both groups
    cat = np.concatenate((np.concatenate((pred[:10, 4:8], cls_prob[:10, 1:2]), 1), extra[:2]), 0)
    assert np.array_equal(part[:n_part], cat[detect_ref.nms(cat, 0.3)])


# ---- refusals of the C entries (no GPU: a refused call returns before any HIP call) ------------------------------------------------
PTR = ctypes.c_void_p(0x1000)      # a non-NULL, 16-byte aligned stand-in: refused calls never dereference it
NULL = None


def test_topk_refusals(hip_lib):
    f = hip_lib.ft_topk_desc_f32
    assert hip_lib.ft_topk_desc_f32_workspace_bytes(21546, 6000) == 0
    assert f(NULL, 0, 0, NULL, NULL, NULL, None) == FT_OK and f(PTR, 10, 0, PTR, PTR, NULL, None) == FT_OK
    assert f(PTR, -1, 1, PTR, PTR, NULL, None) == FT_ERR_INVALID_ARG and f(PTR, 5, -1, PTR, PTR, NULL, None) == FT_ERR_INVALID_ARG
    assert f(PTR, 65537, 10, PTR, PTR, NULL, None) == FT_ERR_UNSUPPORTED
    assert f(PTR, 65536, 16385, PTR, PTR, NULL, None) == FT_ERR_UNSUPPORTED
    assert f(PTR, 10, 11, PTR, PTR, NULL, None) == FT_ERR_UNSUPPORTED                            # k > n
    for args in ((NULL, 10, 5, PTR, PTR), (PTR, 10, 5, NULL, PTR), (PTR, 10, 5, PTR, NULL)):
        assert f(*args, NULL, None) == FT_ERR_INVALID_ARG


def test_proposal_rois_refusals(hip_lib):
    f = hip_lib.ft_proposal_rois_fwd
    assert f(NULL, NULL, NULL, 0, 0, NULL, NULL, None) == FT_OK
    assert f(PTR, PTR, PTR, -1, 4, PTR, PTR, None) == FT_ERR_INVALID_ARG and f(PTR, PTR, PTR, 4, -1, PTR, PTR, None) == FT_ERR_INVALID_ARG
    for args in ((NULL, PTR, PTR, 4, 4, PTR, PTR), (PTR, NULL, PTR, 4, 4, PTR, PTR), (PTR, PTR, NULL, 4, 4, PTR, PTR),
                 (PTR, PTR, PTR, 4, 4, NULL, PTR), (PTR, PTR, PTR, 4, 4, PTR, NULL)):
        assert f(*args, None) == FT_ERR_INVALID_ARG, args
    assert f(PTR, PTR, PTR, 4, 1 << 29, PTR, PTR, None) == FT_ERR_UNSUPPORTED


def test_detect_select_refusals(hip_lib):
    f = lambda cp, pb, R, nr, K, pid, ex, M, ec, ms, th, mk, cap, d, c: hip_lib.ft_detect_select_fwd(cp, pb, R, nr, K, pid, ex, M, ec, ms, th, mk, cap, d, c, None)
    ok = (PTR, PTR, 300, PTR, 3, 1, PTR, 8, NULL, 0.0, 0.3, 0, 308, PTR, PTR)

    def with_(**kw):
        names = ("cp", "pb", "R", "nr", "K", "pid", "ex", "M", "ec", "ms", "th", "mk", "cap", "d", "c")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for bad in (dict(pid=3), dict(pid=-1), dict(K=0), dict(cap=0), dict(R=-1), dict(M=-1), dict(th=float("nan")), dict(ms=float("nan")),
                dict(d=NULL), dict(c=NULL), dict(cp=NULL), dict(pb=NULL), dict(nr=NULL)):
        assert f(*with_(**bad)) == FT_ERR_INVALID_ARG, bad
    assert f(*with_(M=725)) == FT_ERR_UNSUPPORTED and f(*with_(R=1025, M=0)) == FT_ERR_UNSUPPORTED      # R + M > 1024
