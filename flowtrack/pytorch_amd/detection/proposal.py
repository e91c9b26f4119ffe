"""The detector's region stage above the operators: anchors, the proposal layer and the two RoI feature forms.

    generate_anchors_pre   layer_utils/snippets.py + generate_anchors.py, host numpy
    proposal_layer         layer_utils/proposal_layer.py:19-56: decode + clip (ft_rpn_decode_boxes), top-N by a stable
                           descending sort, ft_box_nms (IoU > thresh, capped at post_nms_topN) and the [n,5] blob, with exactly
                           one device -> host read: the kept count
    proposal_layer_device  the same blob without that read: ft_topk_desc_f32 for the sort, ft_box_nms, ft_proposal_rois_fwd into a
                           caller-given [rows,5] buffer; returns device tensors only (the frame step of detect_persons_clip)
    crop_pool_layer        nets/network.py:93-121 on CropAndResizeFunction + F.max_pool2d, NCHW (the training drop-in)
    roi_crop_nhwc          the same values from dense NHWC fp16 / fp32 features in one launch (ft_roi_crop_nhwc_fwd): the
                           [R,pooled,pooled,C] tensor is the input of the layer4 convs (ft_conv2d_fwd, N = R)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from .._lib import FlowtrackHipError, check
from .ops import CropAndResizeFunction, _fp32_cuda, _ptr, _stream, box_nms_sorted

__all__ = ["generate_anchors", "generate_anchors_pre", "decode_boxes", "proposal_layer", "proposal_layer_device", "topk_desc", "crop_pool_layer", "roi_crop_nhwc", "RPN_DEFAULTS"]

#: model/config.py: (RPN_PRE_NMS_TOP_N, RPN_POST_NMS_TOP_N, RPN_NMS_THRESH) per mode
RPN_DEFAULTS = {"TEST": (6000, 300, 0.7), "TRAIN": (12000, 2000, 0.7)}
POOLING_SIZE = 7   # model/config.py: POOLING_SIZE


def _window(w, h, x_ctr, y_ctr):
    """Windows of widths w / heights h (vectors) around one centre, as (x1, y1, x2, y2) rows."""
    w, h = w[:, np.newaxis], h[:, np.newaxis]
    return np.hstack((x_ctr - 0.5 * (w - 1), y_ctr - 0.5 * (h - 1), x_ctr + 0.5 * (w - 1), y_ctr + 0.5 * (h - 1)))


def _centre(a):
    w, h = a[2] - a[0] + 1, a[3] - a[1] + 1
    return w, h, a[0] + 0.5 * (w - 1), a[1] + 0.5 * (h - 1)


def generate_anchors(base_size=16, ratios=(0.5, 1, 2), scales=(8, 16, 32)):
    """The A = len(ratios) * len(scales) base windows around a (0, 0, base_size - 1, base_size - 1) cell: every aspect ratio
    at (rounded) constant area, then every scale of each, ratio-major."""
    ratios, scales = np.asarray(ratios, dtype=np.float64), np.asarray(scales)
    w, h, x_ctr, y_ctr = _centre(np.array([0, 0, base_size - 1, base_size - 1]))
    ws = np.round(np.sqrt(w * h / ratios))
    hs = np.round(ws * ratios)
    by_ratio = _window(ws, hs, x_ctr, y_ctr)
    out = []
    for row in by_ratio:
        w, h, x_ctr, y_ctr = _centre(row)
        out.append(_window(w * scales, h * scales, x_ctr, y_ctr))
    return np.vstack(out)


def generate_anchors_pre(height, width, feat_stride, anchor_scales=(8, 16, 32), anchor_ratios=(0.5, 1, 2)):
    """All anchors of a height x width map, cell-major (x fastest) with the A base windows innermost: (float32 [K*A, 4],
    np.int32 K*A)."""
    base = generate_anchors(ratios=np.array(anchor_ratios), scales=np.array(anchor_scales))
    sx, sy = np.meshgrid(np.arange(0, width) * feat_stride, np.arange(0, height) * feat_stride)
    shifts = np.vstack((sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel())).transpose()
    A, K = base.shape[0], shifts.shape[0]
    anchors = (base.reshape((1, A, 4)) + shifts.reshape((K, 1, 4))).reshape((K * A, 4)).astype(np.float32, copy=False)
    return anchors, np.int32(anchors.shape[0])


def decode_boxes(anchors: torch.Tensor, deltas: torch.Tensor, im_h: float, im_w: float) -> torch.Tensor:
    """ft_rpn_decode_boxes: bbox_transform_inv + clip_boxes of [A,4] anchors / deltas."""
    anchors = _fp32_cuda(anchors, "decode_boxes anchors", (None, 4))
    deltas = _fp32_cuda(deltas, "decode_boxes deltas", (anchors.shape[0], 4))
    if deltas.device != anchors.device:
        raise FlowtrackHipError(f"decode_boxes: anchors on {anchors.device}, deltas on {deltas.device}")
    boxes = torch.empty_like(anchors)
    with torch.cuda.device(anchors.device):
        check(_lib.load().ft_rpn_decode_boxes(_ptr(anchors), _ptr(deltas), anchors.shape[0], float(im_h), float(im_w), _ptr(boxes),
                                              _stream(anchors.device)), "ft_rpn_decode_boxes")
    return boxes


def proposal_layer(rpn_cls_prob, rpn_bbox_pred, im_info, cfg_key, feat_stride, anchors, num_anchors, *, pre_nms_topN=None,
                   post_nms_topN=None, nms_thresh=None):
    """rpn_cls_prob [1,H,W,2A] (foreground scores in the last A channels), rpn_bbox_pred [1,H,W,4A], im_info (height, width,
    ...) on the host, anchors [H*W*A,4] -> (blob [n,5] = (0, x1, y1, x2, y2), scores [n,1]).  Single image, as the reference."""
    if isinstance(cfg_key, bytes):
        cfg_key = cfg_key.decode("utf-8")
    if cfg_key not in RPN_DEFAULTS:
        raise FlowtrackHipError(f"proposal_layer: cfg_key {cfg_key!r} is neither 'TEST' nor 'TRAIN'")
    pre, post, thresh = RPN_DEFAULTS[cfg_key]
    pre = pre if pre_nms_topN is None else int(pre_nms_topN)
    post = post if post_nms_topN is None else int(post_nms_topN)
    thresh = thresh if nms_thresh is None else float(nms_thresh)
    rpn_cls_prob = _fp32_cuda(rpn_cls_prob, "proposal_layer rpn_cls_prob", (1, None, None, 2 * num_anchors))
    rpn_bbox_pred = _fp32_cuda(rpn_bbox_pred, "proposal_layer rpn_bbox_pred", rpn_cls_prob.shape[:3] + (4 * num_anchors,))
    im_h, im_w = float(im_info[0]), float(im_info[1])          # the host's copy: no device read
    scores = rpn_cls_prob[:, :, :, num_anchors:].contiguous().view(-1)
    if isinstance(anchors, np.ndarray):
        anchors = torch.from_numpy(anchors).to(rpn_cls_prob.device)
    proposals = decode_boxes(anchors, rpn_bbox_pred.detach().view(-1, 4), im_h, im_w)
    if proposals.shape[0] != scores.shape[0]:
        raise FlowtrackHipError(f"proposal_layer: {proposals.shape[0]} anchors for {scores.shape[0]} scores")
    scores, order = scores.detach().sort(descending=True, stable=True)   # plumbing; a sort kernel is a follow-up
    if pre > 0:
        order, scores = order[:pre], scores[:pre]
    proposals = proposals[order]
    scores = scores.view(-1, 1)
    keep, count = box_nms_sorted(torch.cat((proposals, scores), 1), thresh, inclusive=False, max_keep=post)
    n = int(count.item())                                      # the one device -> host read
    keep = keep[:n].long()
    proposals, scores = proposals[keep], scores[keep]
    blob = torch.cat((proposals.new_zeros((n, 1)), proposals), 1)
    return blob, scores


def topk_desc(scores: torch.Tensor, k: int):
    """ft_topk_desc_f32: the first k entries of scores.sort(descending=True, stable=True) of an fp32 CUDA vector as (sorted
    float32 [k], order int32 [k]), one launch, nothing read back.  1 <= k <= min(n, 16384), n <= 65536."""
    scores = _fp32_cuda(scores, "topk_desc scores", (None,))
    n, k = scores.shape[0], int(k)
    order = torch.empty(k, dtype=torch.int32, device=scores.device)
    out = torch.empty(k, dtype=torch.float32, device=scores.device)
    lib = _lib.load()
    nbytes = lib.ft_topk_desc_f32_workspace_bytes(n, k)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=scores.device) if nbytes > 0 else None
    with torch.cuda.device(scores.device):
        check(lib.ft_topk_desc_f32(_ptr(scores), n, k, _ptr(order), _ptr(out), _ptr(workspace), _stream(scores.device)), "ft_topk_desc_f32")
    return out, order


def proposal_layer_device(rpn_cls_prob, rpn_bbox_pred, im_info, cfg_key, feat_stride, anchors, num_anchors, rois, *, pre_nms_topN=None,
                          post_nms_topN=None, nms_thresh=None):
    """proposal_layer with every step enqueued and nothing read from the device: the blob goes into the caller's `rois` [rows,5]
    fp32 CUDA buffer (the first n = min(kept, rows) rows; the rest are zeroed) and n stays on the device.  Returns (rois, n_rois
    int32 [1]).  `anchors` is a CUDA tensor; im_info is the host's copy.  The NMS is capped at min(post_nms_topN, rows)."""
    if isinstance(cfg_key, bytes):
        cfg_key = cfg_key.decode("utf-8")
    if cfg_key not in RPN_DEFAULTS:
        raise FlowtrackHipError(f"proposal_layer_device: cfg_key {cfg_key!r} is neither 'TEST' nor 'TRAIN'")
    pre, post, thresh = RPN_DEFAULTS[cfg_key]
    pre = pre if pre_nms_topN is None else int(pre_nms_topN)
    post = post if post_nms_topN is None else int(post_nms_topN)
    thresh = thresh if nms_thresh is None else float(nms_thresh)
    rpn_cls_prob = _fp32_cuda(rpn_cls_prob, "proposal_layer_device rpn_cls_prob", (1, None, None, 2 * num_anchors))
    rpn_bbox_pred = _fp32_cuda(rpn_bbox_pred, "proposal_layer_device rpn_bbox_pred", rpn_cls_prob.shape[:3] + (4 * num_anchors,))
    if not isinstance(rois, torch.Tensor) or not rois.is_cuda or rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] != 5 or \
            rois.shape[0] < 1 or not rois.is_contiguous() or rois.device != rpn_cls_prob.device:
        raise FlowtrackHipError("proposal_layer_device rois: expected a contiguous fp32 CUDA buffer [rows,5], rows >= 1, on the maps' device")
    rows = int(rois.shape[0])
    device = rpn_cls_prob.device
    im_h, im_w = float(im_info[0]), float(im_info[1])          # the host's copy: no device read
    scores = rpn_cls_prob[:, :, :, num_anchors:].contiguous().view(-1)
    anchors = _fp32_cuda(anchors, "proposal_layer_device anchors", (scores.shape[0], 4))
    proposals = decode_boxes(anchors, rpn_bbox_pred.detach().view(-1, 4), im_h, im_w)
    n_all = scores.shape[0]
    n_rois = torch.zeros(1, dtype=torch.int32, device=device)
    if n_all == 0:
        rois.zero_()
        return rois, n_rois
    k = min(pre, n_all) if pre > 0 else n_all
    top_scores, order = topk_desc(scores.detach(), k)
    top = proposals.index_select(0, order)
    keep, count = box_nms_sorted(torch.cat((top, top_scores.view(-1, 1)), 1), thresh, inclusive=False, max_keep=min(post, rows) if post > 0 else rows)
    with torch.cuda.device(device):
        check(_lib.load().ft_proposal_rois_fwd(_ptr(top), _ptr(keep), _ptr(count), k, rows, _ptr(rois), _ptr(n_rois), _stream(device)),
              "ft_proposal_rois_fwd")
    return rois, n_rois


def crop_pool_layer(bottom, rois, max_pool=True, feat_stride=16.0, pooled=POOLING_SIZE):
    """Network._crop_pool_layer: bottom [B,C,H,W], rois [R,5] in image pixels -> [R,C,pooled,pooled]."""
    rois = rois.detach()
    height, width = bottom.size(2), bottom.size(3)

    def div(a, b):
        # the correctly rounded fp32 quotient (a double quotient rounded to fp32 is one): torch divides a CUDA tensor by a
        # Python scalar as a * (1 / b), which is an ulp off for most b and would part this from ft_roi_crop_nhwc_fwd
        return (a.double() / b).float()

    x1, y1 = div(rois[:, 1:2], feat_stride), div(rois[:, 2:3], feat_stride)
    x2, y2 = div(rois[:, 3:4], feat_stride), div(rois[:, 4:5], feat_stride)
    pre_pool = pooled * 2 if max_pool else pooled
    boxes = torch.cat([div(y1, height - 1), div(x1, width - 1), div(y2, height - 1), div(x2, width - 1)], 1)
    crops = CropAndResizeFunction(pre_pool, pre_pool)(bottom, boxes, rois[:, 0].int())
    if max_pool:
        crops = F.max_pool2d(crops, 2, 2)
    return crops


def roi_crop_nhwc(features, rois, feat_stride=16., pooled=POOLING_SIZE, max_pool=False):
    """ft_roi_crop_nhwc_fwd: dense NHWC features [B,H,W,C] (fp16 or fp32, C % 8 == 0, H, W >= 2), rois [R,5] fp32 in image
    pixels -> [R,pooled,pooled,C] in the features' dtype, the values of crop_pool_layer rounded once."""
    if not isinstance(features, torch.Tensor):
        raise FlowtrackHipError(f"roi_crop_nhwc features: expected an fp16 or fp32 CUDA tensor, got {type(features).__name__}")
    if features.dim() != 4:
        raise FlowtrackHipError(f"roi_crop_nhwc features: expected [B,H,W,C], got shape {tuple(features.shape)}")
    if not features.is_cuda or features.dtype not in (torch.float16, torch.float32):
        raise FlowtrackHipError(f"roi_crop_nhwc features: expected an fp16 or fp32 CUDA tensor, got {features.dtype} on {features.device}")
    features = features.contiguous()
    rois = _fp32_cuda(rois, "roi_crop_nhwc rois", (None, 5))
    if rois.device != features.device:
        raise FlowtrackHipError(f"roi_crop_nhwc: features on {features.device}, rois on {rois.device}")
    B, H, W, C = features.shape
    R = rois.shape[0]
    out = torch.empty((R, pooled, pooled, C), dtype=features.dtype, device=features.device)
    with torch.cuda.device(features.device):
        check(_lib.load().ft_roi_crop_nhwc_fwd(_lib.dtype_code(features.dtype), _ptr(features), _ptr(rois), B, H, W, C, R, float(feat_stride),
                                               int(pooled), int(bool(max_pool)), _ptr(out), _stream(features.device)),
              "ft_roi_crop_nhwc_fwd")
    return out
