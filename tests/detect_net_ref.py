"""Restatement of the Faster R-CNN detector network (reference lib/detection: nets/resnet_v1.py, nets/network.py inference half,
model/test.py: im_detect, lib/tracking/net_utils.py: detect) for the tests of detection/nets.py, detection/test.py and
csrc/detect_net_ops.hip.

  head / rpn / region_head / im_detect / detect_persons   a torch-CPU functional forward from a state_dict (fp32, torch's own conv /
                                                          batch_norm / max_pool, the region stage from tests/detect_ref.py)
  blob_ref / rpn_softmax_ref / mean_pool_ref / detections_ref   the four glue kernels, `dtype` = np.float32 (every operation rounded
                                                          separately, the kernels' order) or np.float64
  blob_bound / softmax_bound / mean_pool_bound / detections_bound   what |fp32 kernel - float64 reference| may be, first order in
                                                          u = 2^-24, from counted roundings (derivations at each function)
"""
import numpy as np
import torch
import torch.nn.functional as F

import detect_ref
from detect_ref import EXPF_ULPS, F32, U32

BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
PIXEL_MEANS = np.array([102.9801, 115.9465, 122.7717])              # model/config.py, BGR
BBOX_STDS, BBOX_MEANS = (0.1, 0.1, 0.2, 0.2), (0.0, 0.0, 0.0, 0.0)  # TRAIN.BBOX_NORMALIZE_STDS / _MEANS
U16 = 2.0 ** -11                                                    # unit round-off of fp16
SLACK = 1.01                                                        # second-order terms


# ---- sizes --------------------------------------------------------------------------------------------------------------------
def blob_size(h, w, target_size=600, max_size=1000):
    """model/test.py:40-53: (im_scale, Hb, Wb).  cv2.resize(fx, fy) takes dsize = cvRound(size * f): round half to even."""
    im_scale = float(target_size) / float(min(h, w))
    if np.round(im_scale * max(h, w)) > max_size:
        im_scale = float(max_size) / float(max(h, w))
    return im_scale, int(np.rint(h * im_scale)), int(np.rint(w * im_scale))


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def map_sizes(n):
    """Sizes behind conv1, the max-pool (= layer1), layer2 and layer3 (= layer4) of the Caffe-strided trunk."""
    a = conv_out(n, 7, 2, 3)
    b = conv_out(a, 3, 2, 1)
    c = conv_out(b, 1, 2, 0)
    return a, b, c, conv_out(c, 1, 2, 0)


# ---- the four kernels ---------------------------------------------------------------------------------------------------------
def _axis_table(n_out, scale, size):
    """OpenCV's INTER_LINEAR index / weight table of one axis for float images: (i0, i1, fraction float32)."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * float(scale) - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    lo, hi = s < 0, s >= size - 1
    f[lo | hi] = 0
    s[lo] = 0
    s[hi] = size - 1
    return s, np.minimum(s + 1, size - 1), f


def resize_linear(src, Hb, Wb, scale_y, scale_x, dtype=np.float64):
    """OpenCV's INTER_LINEAR rule for a float image [H,W,C] -> [Hb,Wb,C]: the horizontal pass, then the vertical one, in `dtype`,
    with the fp32 fractions f and the weights 1 - f formed in fp32."""
    src = np.asarray(src).astype(dtype)
    H, W, _ = src.shape
    x0, x1, fx = _axis_table(Wb, scale_x, W)
    y0, y1, fy = _axis_table(Hb, scale_y, H)
    a0, a1 = (F32(1) - fx).astype(dtype)[None, :, None], fx.astype(dtype)[None, :, None]
    b0, b1 = (F32(1) - fy).astype(dtype)[:, None, None], fy.astype(dtype)[:, None, None]
    rows = src[:, x0] * a0 + src[:, x1] * a1                   # [H, Wb, 3]: the horizontal pass
    return (rows[y0] * b0 + rows[y1] * b1).astype(dtype)       # [Hb, Wb, 3]: the vertical pass


def blob_ref(frame, means, Hb, Wb, scale_y, scale_x, dtype=np.float64):
    """ft_detect_blob_fwd: frame u8 [H,W,3] -> [1,3,Hb,Wb].  The float64 means are subtracted in double and the difference
    rounded to fp32 (model/test.py:37-38: `im_orig -= cfg.PIXEL_MEANS` on a float32 image), then resize_linear, then the HWC -> CHW
    transpose of nets/network.py:378."""
    src = (np.asarray(frame).astype(np.float64) - np.asarray(means, dtype=np.float64)).astype(F32)
    out = resize_linear(src, Hb, Wb, scale_y, scale_x, dtype)
    return np.ascontiguousarray(out.transpose(2, 0, 1))[None]


def blob_bound(frame, means):
    """Inputs (fp32 samples s, |s| <= M, fp32 weights with a0 + a1 = 1 up to one rounding of a0) are shared with the reference.
    Horizontal pass fl(fl(s0 a0) + fl(s1 a1)): u |s0 a0| + u |s1 a1| + u |sum| <= 2 u M, plus the rounding of a0 = fl(1 - f): u M.
    The vertical pass carries that 3 u M through weights that sum to 1 and adds 3 u M of its own: 6 u M; 8 u M states it."""
    M = float(np.abs(np.asarray(frame, dtype=np.float64) - np.asarray(means, dtype=np.float64)).max())
    return 8 * U32 * M * SLACK


def rpn_softmax_ref(x, A, dtype=np.float64):
    """ft_rpn_softmax_fwd: x [rows, 2A] -> exp(x - max) / sum over the pairs (a, a + A)."""
    x = np.asarray(x).astype(F32).astype(dtype).reshape(-1, 2, A)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    return (e / e.sum(axis=1, keepdims=True)).reshape(-1, 2 * A)


def softmax_bound(x, axis):
    """exp(x - max) / sum over `axis` of K terms, per row: d = fl(x - m) is off by u |d|, which moves exp(d) by the relative
    u |d|; expf itself by EXPF_ULPS ulps = 2 EXPF_ULPS u; so every term has the relative error r = (2 EXPF_ULPS + |d|max) u.  The sum
    of K positive terms adds (K - 1) u, the division u, and the quotient of two quantities with relative errors r and r + (K - 1) u
    is off by their sum.  Probabilities are <= 1, so the relative figure is the absolute bound."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[axis]
    dmax = x.max(axis=axis, keepdims=True) - x.min(axis=axis, keepdims=True)
    return np.broadcast_to((2 * (2 * EXPF_ULPS + dmax) + K + 1) * U32 * SLACK, x.shape)


def mean_pool_ref(x, dtype=np.float64):
    """ft_rcnn_mean_pool_fwd: x [R,P,P,C] -> [R,C]: sums in x order / P, those summed in y order / P."""
    x = np.asarray(x).astype(F32).astype(dtype)
    R, P, _, C = x.shape
    acc = np.zeros((R, C), dtype=dtype)
    for y in range(P):
        row = np.zeros((R, C), dtype=dtype)
        for xx in range(P):
            row = row + x[:, y, xx]
        acc = acc + row / dtype(P)
    return acc / dtype(P)


def mean_pool_bound(x, out_dtype=np.float32):
    """Per output, with S = sum |x| over the P x P cells: a row sum of P terms rounds P - 1 times (<= (P - 1) u of the row's
    |x| sum), its division once; summing the P row means rounds P - 1 times and the last division once: (2 P) u S / P^2 in all,
    stated with 2 P + 2.  An fp16 result adds its own rounding, 2^-11 |out|."""
    x = np.asarray(x, dtype=np.float64)
    P = x.shape[1]
    mag = np.abs(x).sum(axis=(1, 2)) / (P * P)
    b = (2 * P + 2) * U32 * mag * SLACK
    if out_dtype == np.float16:
        b = b + U16 * (np.abs(x.sum(axis=(1, 2))) / (P * P) + b)
    return b


def detections_ref(cls_score, bbox_pred, rois, stds, means, im_scale, im_h, im_w, dtype=np.float64):
    """ft_rcnn_detections_fwd: (cls_prob [R,K], deltas [R,4K], pred_boxes [R,4K]).  The deltas are fp32 products and sums in both
    flavours (nets/network.py:389 forms them in fp32); float64 forms rois / im_scale and the decode in double, as
    model/test.py:97-104 does with its float64 im_scale."""
    s = np.asarray(cls_score).astype(F32).astype(dtype)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True)
    bp = np.asarray(bbox_pred, dtype=F32)
    R, K = bp.shape[0], bp.shape[1] // 4
    deltas = (bp.reshape(R, K, 4) * np.asarray(stds, dtype=F32) + np.asarray(means, dtype=F32)).astype(F32)
    scale = dtype(F32(im_scale)) if dtype == F32 else dtype(im_scale)
    boxes = np.asarray(rois, dtype=F32)[:, 1:5].astype(dtype) / scale
    one, half = dtype(1), dtype(0.5)
    w, h = boxes[:, 2] - boxes[:, 0] + one, boxes[:, 3] - boxes[:, 1] + one
    cx, cy = boxes[:, 0] + half * w, boxes[:, 1] + half * h
    d = deltas.astype(dtype)
    pcx, pcy = d[:, :, 0] * w[:, None] + cx[:, None], d[:, :, 1] * h[:, None] + cy[:, None]
    pw, ph = np.exp(d[:, :, 2]) * w[:, None], np.exp(d[:, :, 3]) * h[:, None]
    out = np.stack((np.maximum(pcx - half * pw, dtype(0)), np.maximum(pcy - half * ph, dtype(0)),
                    np.minimum(pcx + half * pw, dtype(im_w - 1)), np.minimum(pcy + half * ph, dtype(im_h - 1))), 2)
    return prob, deltas.reshape(R, 4 * K), out.reshape(R, 4 * K)


def detections_bound(bbox_pred, rois, stds, means, im_scale):
    """pred_boxes [R,4K]: detect_ref.decode_bound of the exact boxes rois / im_scale with the (shared, fp32) deltas, plus what the
    fp32 boxes add.  A box edge b = fl(roi / fl(im_scale)) is off by e_b = 2 u |b| (im_scale rounded to fp32, then the division).
    Through bbox_transform_inv, per axis with edges lo, hi: the size s moves by e_s = e_lo + e_hi, the centre by e_lo + 0.5 e_s,
    the decoded centre by |d| e_s + that, the decoded size by exp(ds) e_s, an output edge by the centre's plus half the size's.
    The clip is 1-Lipschitz."""
    bp = np.asarray(bbox_pred, dtype=F32)
    R, K = bp.shape[0], bp.shape[1] // 4
    deltas = (bp.reshape(R, K, 4) * np.asarray(stds, dtype=F32) + np.asarray(means, dtype=F32)).astype(np.float64)
    boxes = np.asarray(rois, dtype=np.float64)[:, 1:5] / float(im_scale)
    e_b = 2 * U32 * np.abs(boxes)
    out = np.zeros((R, K, 4))
    for c in range(K):
        out[:, c] = detect_ref.decode_bound(boxes, deltas[:, c])
        for axis in (0, 1):
            e_s = e_b[:, axis] + e_b[:, axis + 2]
            e_pc = np.abs(deltas[:, c, axis]) * e_s + e_b[:, axis] + 0.5 * e_s
            e_ps = np.exp(deltas[:, c, axis + 2]) * e_s
            out[:, c, axis] += SLACK * (e_pc + 0.5 * e_ps)
            out[:, c, axis + 2] += SLACK * (e_pc + 0.5 * e_ps)
    return out.reshape(R, 4 * K)


# ---- the network, torch CPU ---------------------------------------------------------------------------------------------------
def _bn(sd, name, x):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.0, 1e-5)


def _bottleneck(sd, name, x, s1, s2, sd_stride):
    """One block with conv1 at stride s1, conv2 at s2 and, where the state_dict has one, the shortcut conv at sd_stride."""
    out = F.relu(_bn(sd, name + ".bn1", F.conv2d(x, sd[name + ".conv1.weight"], stride=s1)))
    out = F.relu(_bn(sd, name + ".bn2", F.conv2d(out, sd[name + ".conv2.weight"], stride=s2, padding=1)))
    out = _bn(sd, name + ".bn3", F.conv2d(out, sd[name + ".conv3.weight"]))
    if name + ".downsample.0.weight" in sd:
        x = _bn(sd, name + ".downsample.1", F.conv2d(x, sd[name + ".downsample.0.weight"], stride=sd_stride))
    return F.relu(out + x)


def _layer(sd, li, blocks, x):
    """nets/resnet_v1.py:25-37: layer2.0 / layer3.0 stride on conv1 and the shortcut, layer4.0 has none."""
    for bi in range(blocks):
        s = 2 if (bi == 0 and li in (2, 3)) else 1
        x = _bottleneck(sd, f"resnet.layer{li}.{bi}", x, s, 1, s)
    return x


def head(sd, blob, depth=50):
    """_image_to_head: blob [1,3,H,W] -> net_conv [1,1024,h,w]."""
    sd = {k: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(blob), dtype=torch.float32)
        # nets/network.py:378 feeds the transposed view of the HWC blob: torch runs the trunk in that memory format, whose
        # convolutions sum in another order than the NCHW ones (1e-5 apart on values of 15)
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        x = F.relu(_bn(sd, "resnet.bn1", F.conv2d(x, sd["resnet.conv1.weight"], stride=2, padding=3)))
        x = F.max_pool2d(x, 3, 2, 1)
        for li in (1, 2, 3):
            x = _layer(sd, li, BLOCKS[depth][li - 1], x)
    return x


def rpn(sd, net_conv, A=9):
    """_region_proposal up to the proposal layer: (rpn_cls_score [1,h,w,2A], rpn_cls_prob [1,h,w,2A], rpn_bbox_pred [1,h,w,4A])."""
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(net_conv), dtype=torch.float32)
        r = F.relu(F.conv2d(x, sd["rpn_net.weight"], sd["rpn_net.bias"], padding=1))
        score = F.conv2d(r, sd["rpn_cls_score_net.weight"], sd["rpn_cls_score_net.bias"]).contiguous()
        prob = F.softmax(score.view(1, 2, -1, score.shape[-1]), dim=1).view_as(score).permute(0, 2, 3, 1)
        bbox = F.conv2d(r, sd["rpn_bbox_pred_net.weight"], sd["rpn_bbox_pred_net.bias"]).permute(0, 2, 3, 1)
    return score.permute(0, 2, 3, 1).contiguous().numpy(), prob.contiguous().numpy(), bbox.contiguous().numpy()


def anchors_for(h, w, scales=(8, 16, 32), ratios=(0.5, 1, 2)):
    """layer_utils/snippets.py: generate_anchors_pre at stride 16 (restated in the package: detection/proposal.py; host numpy)."""
    from flowtrack.pytorch_amd.detection.proposal import generate_anchors_pre
    return generate_anchors_pre(h, w, 16, scales, ratios)[0]


def proposals(rpn_cls_prob, rpn_bbox_pred, im_info, A=9, pre=6000, post=300, thresh=0.7, dtype=F32):
    h, w = rpn_cls_prob.shape[1:3]
    return detect_ref.proposal_layer(rpn_cls_prob, rpn_bbox_pred, im_info, anchors_for(h, w), A, pre, post, thresh, dtype)[0]


def region_head(sd, net_conv, rois, depth=50):
    """_crop_pool_layer (crop mode, no max-pool), layer4, the two means, the two FCs: (pool5, fc7, cls_score [R,K], bbox_pred [R,4K]
    BEFORE the un-normalisation)."""
    pool5 = torch.from_numpy(detect_ref.crop_pool(np.asarray(net_conv, dtype=F32), rois, 16.0, 7, False))
    with torch.no_grad():
        fc7 = _layer(sd, 4, BLOCKS[depth][3], pool5).mean(3).mean(2)
        cls_score = F.linear(fc7, sd["cls_score_net.weight"], sd["cls_score_net.bias"])
        bbox_pred = F.linear(fc7, sd["bbox_pred_net.weight"], sd["bbox_pred_net.bias"])
    return pool5.numpy(), fc7.numpy(), cls_score.numpy(), bbox_pred.numpy()


def im_detect(sd, frame, depth=50, target_size=600, max_size=1000, A=9, pre=6000, post=300, thresh=0.7):
    """model/test.py: im_detect on a BGR uint8 frame; a dict of every seam."""
    H, W, _ = frame.shape
    im_scale, Hb, Wb = blob_size(H, W, target_size, max_size)
    blob = blob_ref(frame, PIXEL_MEANS, Hb, Wb, 1.0 / im_scale, 1.0 / im_scale, np.float64).astype(F32)
    im_info = np.array([Hb, Wb, im_scale], dtype=F32)
    net_conv = head(sd, blob, depth).numpy()
    score, prob, bbox = rpn(sd, net_conv, A)
    rois = proposals(prob, bbox, im_info, A, pre, post, thresh)
    _, _, cls_score, bbox_pred = region_head(sd, net_conv, rois, depth)
    cls_prob, deltas, pred_boxes = detections_ref(cls_score, bbox_pred, rois, BBOX_STDS, BBOX_MEANS, im_scale, H, W, np.float64)
    return dict(blob=blob, im_info=im_info, net_conv=net_conv, rpn_cls_score=score, rpn_cls_prob=prob, rpn_bbox_pred=bbox, rois=rois,
                cls_score=cls_score, cls_prob=cls_prob, bbox_pred=deltas, scores=cls_prob, pred_boxes=pred_boxes)


def detect_persons(scores, pred_boxes, person_id, thresh=0.3, prop_dets=None):
    """lib/tracking/net_utils.py:14-34 behind im_detect: the person column, optional extra boxes, NMS on IoU > thresh."""
    dets = np.hstack((pred_boxes[:, 4 * person_id:4 * (person_id + 1)], scores[:, person_id:person_id + 1])).astype(F32)
    if prop_dets is not None:
        dets = np.concatenate((dets, np.asarray(prop_dets, dtype=F32)), axis=0)
    return dets[detect_ref.nms(dets, thresh, inclusive=False)]
