"""The detector's test-time entry points (reference lib/detection/model/test.py:28-109 and lib/tracking/net_utils.py:14-34).

    im_detect(net, im, target_size=600, max_size=1000) -> (scores [R,C], pred_boxes [R,4C]) as numpy
    detect_persons(net, im, person_id, thresh=0.3, prop_dets=None) -> [N,5] (x1, y1, x2, y2, score) as numpy

The frame goes to the device as uint8; ft_detect_blob_fwd subtracts PIXEL_MEANS, resizes (OpenCV's INTER_LINEAR rule) and writes
the trunk plan's staged NCHW input, so no float frame is built or uploaded.  Behind the two plans ft_rcnn_detections_fwd forms the
class probabilities and the clipped per-class boxes.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import FlowtrackHipError, check
from ..hip_ops import current_stream_handle
from .ops import nms

__all__ = ["PIXEL_MEANS", "blob_size", "stage_frame", "im_detect", "detect_persons"]

PIXEL_MEANS = (102.9801, 115.9465, 122.7717)     # model/config.py: PIXEL_MEANS, BGR
TEST_SCALE, TEST_MAX_SIZE = 600, 1000            # model/config.py: TEST.SCALES[0], TEST.MAX_SIZE


def blob_size(h: int, w: int, target_size: int = TEST_SCALE, max_size: int = TEST_MAX_SIZE):
    """model/test.py:40-53: (im_scale, Hb, Wb).  cv2.resize(fx, fy) takes dsize = cvRound(size * f): round half to even."""
    im_scale = float(target_size) / float(min(h, w))
    if np.round(im_scale * max(h, w)) > max_size:
        im_scale = float(max_size) / float(max(h, w))
    return im_scale, int(np.rint(h * im_scale)), int(np.rint(w * im_scale))


def _frame_on(device, im) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or min(t.shape[:2]) < 1:
        raise FlowtrackHipError("im_detect: expected a BGR uint8 [H,W,3] array or tensor")
    return t.to(device).contiguous()


def stage_frame(net, im, target_size: int = TEST_SCALE, max_size: int = TEST_MAX_SIZE):
    """_get_image_blob into the staged input of the frame's trunk plan: (plan, im_info float32 (Hb, Wb, im_scale), im_scale)."""
    device = next(net.parameters()).device
    frame = _frame_on(device, im)
    H, W = int(frame.shape[0]), int(frame.shape[1])
    im_scale, Hb, Wb = blob_size(H, W, target_size, max_size)
    if Hb < 1 or Wb < 1:
        raise FlowtrackHipError(f"im_detect: a {H}x{W} frame at scale {im_scale} leaves no blob")
    plan = net.trunk_plan(Hb, Wb)
    with torch.cuda.device(device):
        check(_lib.load().ft_detect_blob_fwd(frame.data_ptr(), H, W, (ctypes.c_double * 3)(*PIXEL_MEANS), Hb, Wb, 1.0 / im_scale, 1.0 / im_scale,
                                             plan.x_static.data_ptr(), current_stream_handle(device)), "ft_detect_blob_fwd")
    return plan, np.array([Hb, Wb, im_scale], dtype=np.float32), im_scale, (H, W)


def im_detect(net, im, target_size: int = TEST_SCALE, max_size: int = TEST_MAX_SIZE):
    """model/test.py:88-109 with BBOX_REG: scores = cls_prob [R,C]; pred_boxes [R,4C] = bbox_transform_inv of the un-normalised
    deltas against rois / im_scale, clipped as _clip_boxes clips (x1, y1 only raised, x2, y2 only lowered)."""
    net.eval()
    plan, im_info, _, shape = stage_frame(net, im, target_size, max_size)
    p = net.detect_staged(plan, im_info, frame_shape=shape)
    return p["cls_prob"].cpu().numpy(), p["pred_boxes"].cpu().numpy()


def detect_persons(net, im, person_id: int, thresh: float = 0.3, prop_dets=None, target_size: int = TEST_SCALE, max_size: int = TEST_MAX_SIZE):
    """lib/tracking/net_utils.py:14-34 (`detect`, its `prop_dets != None` test on an array stated as `is not None`): the person
    column of im_detect, optionally with extra boxes `prop_dets` [M,5], through detection.ops.nms (IoU > thresh suppresses)."""
    net.eval()
    plan, im_info, _, shape = stage_frame(net, im, target_size, max_size)
    p = net.detect_staged(plan, im_info, frame_shape=shape)
    dets = torch.cat((p["pred_boxes"][:, 4 * person_id:4 * (person_id + 1)], p["cls_prob"][:, person_id:person_id + 1]), 1)
    if prop_dets is not None:
        extra = torch.as_tensor(np.asarray(prop_dets, dtype=np.float32) if not isinstance(prop_dets, torch.Tensor) else prop_dets)
        dets = torch.cat((dets, extra.to(device=dets.device, dtype=torch.float32).reshape(-1, 5)), 0)
    dets = dets.contiguous()
    keep = nms(dets, thresh)
    return dets[keep].cpu().numpy()
