"""Plain numpy restatements of the detector's clip-pass kernels (csrc/detect_pass_ops.hip): every result is fully determined (a
unique integer key, fp32 expressions rounded one by one), so the GPU tests compare bit for bit."""
import numpy as np

import detect_ref

F32 = np.float32
TOPK_MAX_N, TOPK_MAX_K, SELECT_MAX = 65536, 16384, 1024


def order_key(scores):
    """The documented order key of ft_topk_desc_f32 as uint32: a larger key sorts earlier.  NaN -> the largest key, -0.0 -> the key
    of +0.0, negative values with their bits inverted, the others with the sign bit set."""
    s = np.ascontiguousarray(scores, dtype=F32).reshape(-1)
    u = s.view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(s)] = np.uint32(0xFFFFFFFF)
    return key


def topk_ref(scores, k):
    """(sorted float32 [k], order int32 [k]): a stable arg-sort of the key, descending = ascending (-(key), index)."""
    s = np.ascontiguousarray(scores, dtype=F32).reshape(-1)
    key = order_key(s).astype(np.int64)
    order = np.argsort(-key, kind="stable")[:k]
    return s[order], order.astype(np.int32)


def proposal_rois_ref(boxes, keep, count, rows):
    """ft_proposal_rois_fwd: (rois float32 [rows,5], n_rois)."""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    m = len(boxes)
    c = min(max(int(count), 0), rows, m)
    rois = np.zeros((rows, 5), dtype=F32)
    for j in range(c):
        if 0 <= int(keep[j]) < m:
            rois[j, 1:] = boxes[int(keep[j])]
    return rois, c


def select_ref(cls_prob, pred_boxes, n_rois, person_id, extra, extra_count, min_score, thresh, max_keep, cap):
    """ft_detect_select_fwd: (dets float32 [cap,5] with zeros past the count, count)."""
    cls_prob = np.asarray(cls_prob, dtype=F32)
    R, K = cls_prob.shape
    nr = min(max(int(n_rois), 0), R)
    p = person_id
    cand = np.concatenate((np.asarray(pred_boxes, dtype=F32).reshape(R, 4 * K)[:nr, 4 * p:4 * p + 4], cls_prob[:nr, p:p + 1]), 1)
    if extra is not None and len(extra):
        extra = np.asarray(extra, dtype=F32).reshape(-1, 5)
        ne = len(extra) if extra_count is None else min(max(int(extra_count), 0), len(extra))
        cand = np.concatenate((cand, extra[:ne]), 0)
    cand = cand[~(cand[:, 4] < F32(min_score))]                       # a NaN score is not below anything
    order = np.argsort(-order_key(cand[:, 4]).astype(np.int64), kind="stable")
    cand = cand[order]
    limit = cap if max_keep <= 0 or max_keep > cap else max_keep
    keep, cnt = detect_ref.nms_sorted(cand, thresh, False, limit)
    dets = np.zeros((cap, 5), dtype=F32)
    dets[:cnt] = cand[keep[:cnt]]
    return dets, cnt
