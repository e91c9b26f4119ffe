"""Restatement of the VGG16 Faster R-CNN detector (reference lib/detection: nets/vgg16.py over torchvision's VGG config D, the
inference half of nets/network.py, model/test.py: im_detect) and the references of csrc/vgg_ops.hip, for the tests of
detection.nets.vgg16.

  head / region_head / im_detect   a torch-CPU functional forward from a state_dict (fp32); the RPN, the proposal layer and the
                                   detections come from tests/detect_net_ref.py and tests/detect_ref.py, which do not depend on the trunk
  maxpool_ref                      nn.MaxPool2d(2, 2) on an NHWC array, numpy
  fc_ref                           y = act(x . W^T + bias) in float64
  fc_exact_case / FC_EXACT_CASES   integer data on which every product, partial sum and result of ft_fc_fwd is exact
  fc_bound / two_layer_bound       what |fp16 FC - float64 reference| may be (conv_bound.derived_bound), alone and behind another FC
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import detect_net_ref as R
import detect_ref
from conv_bound import derived_bound
from detect_ref import F32
from flowtrack.pytorch_amd import synth

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # vgg.features indices of the convs; a ReLU follows each
POOLS = (4, 9, 16, 23)                                        # the max-pools that run (nets/vgg16.py:38 drops features.30)


def map_sizes(n):
    """Sizes behind the four pools: floor halving."""
    return n // 2, n // 4, n // 8, n // 16


def head(sd, blob):
    """_image_to_head: blob [1,3,H,W] -> net_conv [1,512,h,w]."""
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(blob), dtype=torch.float32)
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # the memory format nets/network.py:378 feeds (detect_net_ref.head)
        for i in range(30):
            if i in CONVS:
                x = F.relu(F.conv2d(x, sd[f"vgg.features.{i}.weight"], sd[f"vgg.features.{i}.bias"], padding=1))
            elif i in POOLS:
                x = F.max_pool2d(x, 2, 2)
    return x


def region_head(sd, net_conv, rois):
    """_crop_pool_layer (crop mode WITH the 2x2 max-pool, nets/network.py:93), pool5.view(R, -1), classifier.0 / .3 + ReLU, the two
    FCs: (pool5, fc7, cls_score [R,K], bbox_pred [R,4K] BEFORE the un-normalisation)."""
    pool5 = torch.from_numpy(detect_ref.crop_pool(np.asarray(net_conv, dtype=F32), rois, 16.0, 7, True))
    with torch.no_grad():
        fc6 = F.relu(F.linear(pool5.reshape(pool5.shape[0], -1), sd["vgg.classifier.0.weight"], sd["vgg.classifier.0.bias"]))
        fc7 = F.relu(F.linear(fc6, sd["vgg.classifier.3.weight"], sd["vgg.classifier.3.bias"]))
        cls_score = F.linear(fc7, sd["cls_score_net.weight"], sd["cls_score_net.bias"])
        bbox_pred = F.linear(fc7, sd["bbox_pred_net.weight"], sd["bbox_pred_net.bias"])
    return pool5.numpy(), fc7.numpy(), cls_score.numpy(), bbox_pred.numpy()


def proposals(rpn_cls_prob, rpn_bbox_pred, im_info, A=9, pre=6000, post=300, thresh=0.7):
    """detect_ref.proposal_layer with the decode in torch fp32, in the operation order of model/bbox_transform.py:40-59.  This
    trunk's box deltas reach 0.8 on anchors hundreds of pixels wide, where one ulp between numpy's and torch's fp32 exp moves a box
    edge by more than the 1e-5 the golden's generator asks of this restatement; detect_ref.decode_boxes (numpy) stays the
    reference of the GPU tests, which compare inside decode_bound."""
    h, w = rpn_cls_prob.shape[1:3]
    a = torch.from_numpy(np.asarray(R.anchors_for(h, w), dtype=F32))
    d = torch.from_numpy(np.ascontiguousarray(np.asarray(rpn_bbox_pred, dtype=F32).reshape(-1, 4)))
    widths, heights = a[:, 2] - a[:, 0] + 1.0, a[:, 3] - a[:, 1] + 1.0
    cx, cy = a[:, 0] + 0.5 * widths, a[:, 1] + 0.5 * heights
    pcx, pcy = d[:, 0] * widths + cx, d[:, 1] * heights + cy
    pw, ph = torch.exp(d[:, 2]) * widths, torch.exp(d[:, 3]) * heights
    xmax, ymax = float(im_info[1]) - 1, float(im_info[0]) - 1
    boxes = torch.stack(((pcx - 0.5 * pw).clamp(0, xmax), (pcy - 0.5 * ph).clamp(0, ymax), (pcx + 0.5 * pw).clamp(0, xmax),
                         (pcy + 0.5 * ph).clamp(0, ymax)), 1).numpy()
    scores = np.asarray(rpn_cls_prob, dtype=F32)[:, :, :, A:].reshape(-1)
    order = np.argsort(-scores, kind="stable")[:pre]
    dets = np.concatenate((boxes[order], scores[order, None]), 1)
    keep, cnt = detect_ref.nms_sorted(dets, thresh, False, post)
    return np.concatenate((np.zeros((cnt, 1), dtype=F32), dets[keep[:cnt], :4]), 1)


def im_detect(sd, frame, target_size=600, max_size=1000, A=9, pre=6000, post=300, thresh=0.7):
    """model/test.py: im_detect on a BGR uint8 frame; a dict of every seam (detect_net_ref.im_detect with this trunk)."""
    H, W, _ = frame.shape
    im_scale, Hb, Wb = R.blob_size(H, W, target_size, max_size)
    blob = R.blob_ref(frame, R.PIXEL_MEANS, Hb, Wb, 1.0 / im_scale, 1.0 / im_scale, np.float64).astype(F32)
    im_info = np.array([Hb, Wb, im_scale], dtype=F32)
    net_conv = head(sd, blob).numpy()
    score, prob, bbox = R.rpn(sd, net_conv, A)
    rois = proposals(prob, bbox, im_info, A, pre, post, thresh)
    _, fc7, cls_score, bbox_pred = region_head(sd, net_conv, rois)
    cls_prob, deltas, pred_boxes = R.detections_ref(cls_score, bbox_pred, rois, R.BBOX_STDS, R.BBOX_MEANS, im_scale, H, W, np.float64)
    return dict(blob=blob, im_info=im_info, net_conv=net_conv, rpn_cls_score=score, rpn_cls_prob=prob, rpn_bbox_pred=bbox, rois=rois,
                fc7=fc7, cls_score=cls_score, cls_prob=cls_prob, bbox_pred=deltas, scores=cls_prob, pred_boxes=pred_boxes)


# ---- the two kernels ----------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """x [N,H,W,C] -> [N,H//2,W//2,C]: the max of each 2x2 window; the last row / column of an odd map is not read."""
    N, H, W, C = x.shape
    v = x[:, :H // 2 * 2, :W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C)
    return v.max(axis=(2, 4))


def fc_ref(x, w, bias=None, relu=False):
    """float64 y = act(x . W^T + bias): (y, pre-activation)."""
    pre = np.asarray(x, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T
    if bias is not None:
        pre = pre + np.asarray(bias, dtype=np.float64)
    return (np.maximum(pre, 0.0) if relu else pre), pre


#: (R, K, N) of the exact cases: R in {1, 17, 300} x {one K-step, 67 K-steps (no K split of the kernel's divides a prime), the
#: fc6 K at 64 outputs, the fc7 shape}; 64 is the smallest N the kernel takes.  Then the sizes at which the kernel takes another
#: path: 64 / 65 rows (the one-tile and the five-tile row forms), 321 rows (two row chunks), N = 192 (a workgroup with an idle
#: wave pair next to a full one)
FC_EXACT_CASES = tuple((r, k, n) for r in (1, 17, 300) for (k, n) in ((64, 64), (4288, 64), (25088, 64), (4096, 4096))) + \
    ((64, 4288, 64), (65, 4288, 64), (321, 4288, 192))
FC_EXACT_MAX = 2048           # integers up to here are exact in fp16


@functools.lru_cache(maxsize=None)
def fc_exact_case(r, k, n):
    """(x int8 [r,k] in {-2..2}, w int8 [n,k] in {-1,0,1}, bias int32 [n] in [-8, 8]).  About min(k / 2, 512) weights per output are
    non-zero: a pre-activation is a sum of that many terms of variance 2, so its standard deviation is at most 32 and 2048 is 60 of
    them away.  Every product and partial sum is an integer far below 2^24: exact in fp32 whatever the summation order; every
    result is an integer of magnitude <= 2048: exact in fp16."""
    name = f"fc_exact_{r}_{k}_{n}"
    x = (np.floor(synth.uniform01(7, name + ".x", (r, k)) * 5.0) - 2.0).astype(np.int8)
    u = synth.uniform01(7, name + ".w", (n, k))
    p = min(0.5, 512.0 / k)
    w = np.where(u < p / 2, -1, np.where(u < p, 1, 0)).astype(np.int8)
    x[:, 0], x[:, -1], w[:, 0], w[:, -1] = 1, 2, 1, -1       # every result holds a live product of the first and of the last k
    bias = (np.floor(synth.uniform01(7, name + ".b", (n,)) * 17.0) - 8.0).astype(np.int32)
    return x, w, bias


@functools.lru_cache(maxsize=None)
def fc_exact_ref(r, k, n):
    """The float64 pre-activation of the case (an integer array)."""
    x, w, bias = fc_exact_case(r, k, n)
    return fc_ref(x, w, bias)[1]


def fc_bound(x16, w16, bias, relu=True):
    """One fp16 FC with fp32 accumulation against float64 on the same fp16 operands: (bound, want, pre-activation), all [R,N]
    float64 tensors.  conv_bound.derived_bound with the bias add as the one further fp32 operation."""
    x, w = torch.as_tensor(x16).double(), torch.as_tensor(w16).double()
    b = torch.as_tensor(bias).double()
    dot = x @ w.T
    S = x.abs() @ w.abs().T
    pre = dot + b
    want = pre.clamp(min=0) if relu else pre
    v = lambda t: t[:, :, None, None]
    bound = derived_bound(x.shape[1], v(S), v(dot), torch.ones(w.shape[0], dtype=torch.float64), v(want), extra=(v(pre),))
    return bound[:, :, 0, 0], want, pre


def two_layer_bound(x16, w1_16, b1, w2_16, b2):
    """fc7 = relu(W2 relu(W1 x + b1) + b2) with fp16 layers against float64 on the same fp16 input and weights: (bound, want).
    The first layer's output is off by at most e1 = fc_bound; the second layer sees an input within e1 of the exact one, which moves
    its exact result by at most |W2| e1 (ReLU is 1-Lipschitz) and its own rounding bound is taken at the larger magnitudes
    S2 = (|h| + e1) |W2|^T, |pre2| + |W2| e1."""
    e1, h, _ = fc_bound(x16, w1_16, b1)
    w2 = torch.as_tensor(w2_16).double()
    b2 = torch.as_tensor(b2).double()
    carried = e1 @ w2.abs().T
    dot = h @ w2.T
    pre = dot + b2
    want = pre.clamp(min=0)
    S = (h.abs() + e1) @ w2.abs().T
    v = lambda t: t[:, :, None, None]
    own = derived_bound(w2.shape[1], v(S), v(dot.abs() + carried), torch.ones(w2.shape[0], dtype=torch.float64), v(want.abs() + carried),
                        extra=(v(pre.abs() + carried),))
    return own[:, :, 0, 0] + carried, want
