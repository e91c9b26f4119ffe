"""Plain numpy restatements of the detector's region-stage operators (csrc/detect_ops.hip, detection/ops.py, detection/proposal.py).

Two flavours, chosen by `dtype`:
  np.float32  every operation rounded separately, in the order the kernels (and the reference's CUDA kernels) form them: the
              BIT-EXACT comparisons
  np.float64  the same formulas in double: the bounded comparisons (decode, the float gradients)
numpy rounds each fp32 operation once, so `a * b + c` here is two roundings, as in the kernels (which forbid FMA contraction).
Python loops over boxes / bins are fine at the tests' sizes.
"""
import numpy as np

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)          # 2^-23: one ulp of 1.0
U32 = EPS32 / 2                                  # unit round-off of a correctly rounded fp32 operation
EXPF_ULPS = 2.0                                  # allowance for expf (device libm and torch's CPU exp are both specified <= 1 ulp)


# ---- NMS ----------------------------------------------------------------------------------------------------------------------
def iou(a, b, dtype=F32):
    """devIoU: +1 widths, Sa + Sb - inter in that order."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    one, zero = dtype(1), dtype(0)
    left, right = max(a[0], b[0]), min(a[2], b[2])
    top, bottom = max(a[1], b[1]), min(a[3], b[3])
    w, h = max(right - left + one, zero), max(bottom - top + one, zero)
    inter = w * h
    sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    sb = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    with np.errstate(all="ignore"):
        return inter / (sa + sb - inter)


def iou_matrix(boxes, dtype=F32):
    """All pairs at once, the same expression per element."""
    b = np.asarray(boxes, dtype=dtype)[:, :4]
    one, zero = dtype(1), dtype(0)
    left, right = np.maximum(b[:, None, 0], b[None, :, 0]), np.minimum(b[:, None, 2], b[None, :, 2])
    top, bottom = np.maximum(b[:, None, 1], b[None, :, 1]), np.minimum(b[:, None, 3], b[None, :, 3])
    w, h = np.maximum(right - left + one, zero), np.maximum(bottom - top + one, zero)
    inter = w * h
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    with np.errstate(all="ignore"):
        return inter / (area[:, None] + area[None, :] - inter)


def nms_sorted(dets, thresh, inclusive=False, max_keep=0):
    """ft_box_nms on score-descending dets [n,5]: (keep int32[n] with -1 past the count, count).  Box i is kept iff no earlier
    kept box marked it; inclusive: IoU >= thresh suppresses (nms.c), else IoU > thresh (the CUDA path)."""
    dets = np.asarray(dets, dtype=F32).reshape(-1, 5)
    n = len(dets)
    m = iou_matrix(dets)
    hit = (m >= F32(thresh)) if inclusive else (m > F32(thresh))
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if max_keep > 0 and len(keep) >= max_keep:
            break
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= hit[i, i + 1:]
    out = np.full(n, -1, dtype=np.int32)
    out[:len(keep)] = keep
    return out, len(keep)


def nms(dets, thresh, inclusive=False):
    """pth_nms: stable descending sort by score, then the sweep; indices into `dets` in kept order."""
    dets = np.asarray(dets, dtype=F32).reshape(-1, 5)
    order = np.argsort(-dets[:, 4], kind="stable")
    keep, cnt = nms_sorted(dets[order], thresh, inclusive)
    return order[keep[:cnt]]


# ---- RoI pooling --------------------------------------------------------------------------------------------------------------
def round_half_away(v):
    """C's round(): halves go away from zero (np.round goes to even)."""
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def roi_batch_index(v, B):
    """The reference's `int roi_batch_ind = rois[0]`: truncation.  Anything outside [0, B) is 'no image'."""
    b = int(np.trunc(v)) if np.isfinite(v) else -1
    return b if 0 <= b < B else -1


def roi_pool(features, rois, spatial_scale, ph, pw):
    """ROIPoolForward: (out float32 [R,C,ph,pw], argmax int32 [R,C,ph,pw]); a RoI of no image gives zeros / -1."""
    features = np.asarray(features, dtype=F32)
    rois = np.asarray(rois, dtype=F32).reshape(-1, 5)
    B, C, H, W = features.shape
    R = len(rois)
    out = np.zeros((R, C, ph, pw), dtype=F32)
    arg = np.full((R, C, ph, pw), -1, dtype=np.int32)
    scale = F32(spatial_scale)
    for r in range(R):
        b = roi_batch_index(rois[r, 0], B)
        if b < 0:
            continue
        sw, sh, ew, eh = (round_half_away(rois[r, k] * scale) for k in (1, 2, 3, 4))     # the product is fp32
        rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
        bin_h, bin_w = F32(rh) / F32(ph), F32(rw) / F32(pw)
        for i in range(ph):
            hs = min(max(int(np.floor(F32(i) * bin_h)) + sh, 0), H)
            he = min(max(int(np.ceil(F32(i + 1) * bin_h)) + sh, 0), H)
            for j in range(pw):
                ws = min(max(int(np.floor(F32(j) * bin_w)) + sw, 0), W)
                we = min(max(int(np.ceil(F32(j + 1) * bin_w)) + sw, 0), W)
                if he <= hs or we <= ws:
                    continue                                     # empty bin: 0, arg-max -1
                win = features[b, :, hs:he, ws:we].reshape(C, -1)
                k = np.argmax(win, axis=1)                       # first occurrence of the maximum, row-major: the strict `>`
                out[r, :, i, j] = win[np.arange(C), k]
                hh, ww = hs + k // (we - ws), ws + k % (we - ws)
                arg[r, :, i, j] = (np.arange(C) * H + hh) * W + ww
    return out, arg


def roi_pool_bwd(grad_out, rois, argmax, shape, dtype=np.float64):
    """Each grad_out element goes to the arg-max element of the RoI's own image.  Returns (grad_in in `dtype`, the number of
    terms per element, the sum of their magnitudes): the last two make the bound of a float comparison."""
    B, C, H, W = shape
    g = np.zeros((B, C * H * W), dtype=dtype)
    terms = np.zeros((B, C * H * W), dtype=np.int64)
    mag = np.zeros((B, C * H * W), dtype=np.float64)
    rois = np.asarray(rois, dtype=F32).reshape(-1, 5)
    for r in range(len(rois)):
        b = roi_batch_index(rois[r, 0], B)
        if b < 0:
            continue
        a, go = argmax[r].ravel(), np.asarray(grad_out[r]).ravel()
        ok = (a >= 0) & (a < C * H * W)
        np.add.at(g[b], a[ok], go[ok].astype(dtype))
        np.add.at(terms[b], a[ok], 1)
        np.add.at(mag[b], a[ok], np.abs(go[ok].astype(np.float64)))
    return g.reshape(shape), terms.reshape(shape), mag.reshape(shape)


# ---- crop_and_resize ----------------------------------------------------------------------------------------------------------
def crop_axis(lo, hi, crop, size, dtype=F32):
    """One axis of the sampling grid: (inside bool[crop], i0 int[crop], i1 int[crop], lerp dtype[crop])."""
    lo, hi, last = dtype(lo), dtype(hi), dtype(size - 1)
    o = np.arange(crop).astype(dtype)
    with np.errstate(all="ignore"):
        if crop > 1:
            step = (hi - lo) * last / dtype(crop - 1)
            pos = lo * last + o * step
        else:
            pos = np.full(1, dtype(0.5) * (lo + hi) * last, dtype=dtype)
        inside = (pos >= 0) & (pos <= last)                      # a NaN is outside
    safe = np.where(inside, pos, dtype(0))
    i0, i1 = np.floor(safe).astype(np.int64), np.ceil(safe).astype(np.int64)
    return inside, i0, i1, (safe - i0.astype(dtype)).astype(dtype)


def crop_and_resize(image, boxes, box_ind, ch, cw, extrapolation_value=0.0, dtype=F32):
    """CropAndResizeKernel: [R,C,ch,cw]; the x-lerps first, then top + (bottom - top) * y_lerp; all-zero for no image."""
    image = np.asarray(image).astype(dtype)
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    B, C, H, W = image.shape
    R = len(boxes)
    out = np.zeros((R, C, ch, cw), dtype=dtype)
    for r in range(R):
        b = int(box_ind[r])
        if not 0 <= b < B:
            continue
        y1, x1, y2, x2 = boxes[r]
        iny, y0, yb, ly = crop_axis(y1, y2, ch, H, dtype)
        inx, x0, xb, lx = crop_axis(x1, x2, cw, W, dtype)
        img = image[b]
        tl, tr = img[:, y0][:, :, x0], img[:, y0][:, :, xb]
        bl, br = img[:, yb][:, :, x0], img[:, yb][:, :, xb]
        with np.errstate(all="ignore"):
            top = tl + (tr - tl) * lx[None, None, :]
            bottom = bl + (br - bl) * lx[None, None, :]
            val = top + (bottom - top) * ly[None, :, None]
        inside = iny[:, None] & inx[None, :]
        out[r] = np.where(inside[None], val, dtype(extrapolation_value))
    return out


def crop_and_resize_bwd(grad_out, boxes, box_ind, shape, dtype=np.float64):
    """CropAndResizeBackpropImageKernel.  The sampling geometry (neighbours, lerps) is the fp32 one of the forward pass; the four
    weights (1 - lerp) * ... and their sums are formed in `dtype`.  Returns (grad_image, terms per element, sum of |term|)."""
    B, C, H, W = shape
    grad_out = np.asarray(grad_out)
    R, _, ch, cw = grad_out.shape
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    g = np.zeros(shape, dtype=dtype)
    terms = np.zeros(shape, dtype=np.int64)
    mag = np.zeros(shape, dtype=np.float64)
    one = dtype(1)
    for r in range(R):
        b = int(box_ind[r])
        if not 0 <= b < B:
            continue
        y1, x1, y2, x2 = boxes[r]
        iny, y0, yb, ly = crop_axis(y1, y2, ch, H, F32)
        inx, x0, xb, lx = crop_axis(x1, x2, cw, W, F32)
        ly, lx = ly.astype(dtype), lx.astype(dtype)
        for y in np.nonzero(iny)[0]:
            for x in np.nonzero(inx)[0]:
                go = grad_out[r, :, y, x].astype(dtype)
                dtop, dbot = (one - ly[y]) * go, ly[y] * go
                for yy, xx, v in ((y0[y], x0[x], (one - lx[x]) * dtop), (y0[y], xb[x], lx[x] * dtop),
                                  (yb[y], x0[x], (one - lx[x]) * dbot), (yb[y], xb[x], lx[x] * dbot)):
                    g[b, :, yy, xx] += v
                    terms[b, :, yy, xx] += 1
                    mag[b, :, yy, xx] += np.abs(v.astype(np.float64))
    return g, terms, mag


def roi_boxes(rois, H, W, feat_stride=16.0):
    """_crop_pool_layer's box arithmetic in fp32: x / feat_stride, then / (W - 1) and / (H - 1); (boxes [R,4], box_ind [R])."""
    rois = np.asarray(rois, dtype=F32).reshape(-1, 5)
    s = F32(feat_stride)
    x1, y1, x2, y2 = (rois[:, k] / s for k in (1, 2, 3, 4))
    boxes = np.stack((y1 / F32(H - 1), x1 / F32(W - 1), y2 / F32(H - 1), x2 / F32(W - 1)), 1).astype(F32)
    return boxes, np.trunc(rois[:, 0]).astype(np.int64)


def max_pool_2x2(x):
    """F.max_pool2d(x, 2, 2) on [R,C,2p,2p]: a later value replaces the running one only when it is greater."""
    a, b, c, d = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
    m = a.copy()
    for v in (b, c, d):
        m = np.where(v > m, v, m)
    return m


def crop_pool(features_nchw, rois, feat_stride=16.0, pooled=7, max_pool=False):
    """Network._crop_pool_layer in fp32 on NCHW features: [R,C,pooled,pooled]."""
    features_nchw = np.asarray(features_nchw, dtype=F32)
    _, _, H, W = features_nchw.shape
    boxes, ind = roi_boxes(rois, H, W, feat_stride)
    pre = 2 * pooled if max_pool else pooled
    crops = crop_and_resize(features_nchw, boxes, ind, pre, pre, 0.0, F32)
    return max_pool_2x2(crops) if max_pool else crops


# ---- RPN decode ---------------------------------------------------------------------------------------------------------------
def decode_boxes(anchors, deltas, im_h, im_w, dtype=np.float64):
    """bbox_transform_inv + clip_boxes on [A,4] anchors / deltas, in `dtype`."""
    a, d = np.asarray(anchors).astype(dtype), np.asarray(deltas).astype(dtype)
    one, half = dtype(1), dtype(0.5)
    w, h = a[:, 2] - a[:, 0] + one, a[:, 3] - a[:, 1] + one
    cx, cy = a[:, 0] + half * w, a[:, 1] + half * h
    pcx, pcy = d[:, 0] * w + cx, d[:, 1] * h + cy
    pw, ph = np.exp(d[:, 2]) * w, np.exp(d[:, 3]) * h
    out = np.stack((pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph), 1)
    hi = np.array([im_w - 1, im_h - 1, im_w - 1, im_h - 1], dtype=dtype)
    return np.minimum(np.maximum(out, dtype(0)), hi)


def decode_bound(anchors, deltas):
    """Per-coordinate bound [A,4] (pixels) on |fp32 decode - exact decode|, first order in u = 2^-24, from the roundings of
    bbox_transform_inv (model/bbox_transform.py:40-59); the clip is 1-Lipschitz with exact limits and adds nothing.
    Per axis, with s = size (w or h), lo / hi the anchor's edges, d the centre delta, e = exp(size delta):
      s   = fl(fl(hi - lo) + 1)                 e_s   = u (|hi - lo| + |s|)
      c   = fl(lo + 0.5 s)        (0.5 * exact)  e_c   = 0.5 e_s + u |c|
      pc  = fl(fl(d s) + c)                     e_pc  = |d| e_s + u |d s| + e_c + u |pc|
      ps  = fl(expf(.) s)                       e_ps  = e (e_s + (2 EXPF_ULPS + 1) u |s|)     (1 ulp <= 2 u relative)
      out = fl(pc -+ 0.5 ps)                    e_out = e_pc + 0.5 e_ps + u |out|
    times 1.01 for the second-order terms."""
    a, d = np.asarray(anchors, dtype=np.float64), np.asarray(deltas, dtype=np.float64)
    u = U32
    bound = np.zeros((len(a), 4))
    for axis in (0, 1):
        lo, hi, dc, ds = a[:, axis], a[:, axis + 2], d[:, axis], d[:, axis + 2]
        s = hi - lo + 1
        e_s = u * (np.abs(hi - lo) + np.abs(s))
        c = lo + 0.5 * s
        e_c = 0.5 * e_s + u * np.abs(c)
        pc = dc * s + c
        e_pc = np.abs(dc) * e_s + u * np.abs(dc * s) + e_c + u * np.abs(pc)
        e = np.exp(ds)
        ps = e * s
        e_ps = e * (e_s + (2 * EXPF_ULPS + 1) * u * np.abs(s))
        for col, out in ((axis, pc - 0.5 * ps), (axis + 2, pc + 0.5 * ps)):
            bound[:, col] = 1.01 * (e_pc + 0.5 * e_ps + u * np.abs(out))
    return bound


def sum_bound(terms, mag, per_term_roundings=0):
    """|fp32 sum in any order - exact sum| <= (terms + 1 + per_term_roundings) * eps * sum |term|: a sum of n terms rounds n - 1
    times (each by at most u = eps / 2 of a partial sum <= sum |term|); `per_term_roundings` counts the roundings that formed
    each term.  The factor eps (not u) and the + 1 are slack over the first-order figure."""
    return (terms + 1 + per_term_roundings) * EPS32 * mag


# ---- proposal layer -----------------------------------------------------------------------------------------------------------
def proposal_layer(rpn_cls_prob, rpn_bbox_pred, im_info, anchors, num_anchors, pre_nms_topN, post_nms_topN, nms_thresh, dtype=F32):
    """layer_utils/proposal_layer.py: decode + clip, top-N by a stable descending sort, NMS (IoU > thresh), the first
    post_nms_topN survivors: (blob [n,5], scores [n,1], order of the kept boxes among all anchors)."""
    scores = np.asarray(rpn_cls_prob, dtype=F32)[:, :, :, num_anchors:].reshape(-1)
    boxes = decode_boxes(anchors, np.asarray(rpn_bbox_pred, dtype=F32).reshape(-1, 4), im_info[0], im_info[1], dtype).astype(F32)
    order = np.argsort(-scores, kind="stable")
    if pre_nms_topN > 0:
        order = order[:pre_nms_topN]
    dets = np.concatenate((boxes[order], scores[order, None]), 1)
    keep, cnt = nms_sorted(dets, nms_thresh, False, post_nms_topN)
    keep = keep[:cnt]
    blob = np.concatenate((np.zeros((cnt, 1), dtype=F32), dets[keep, :4]), 1)
    return blob, dets[keep, 4:5], order[keep]
