"""The detector's test-time entry points (reference lib/detection/model/test.py:28-109 and lib/tracking/net_utils.py:14-34).

    im_detect(net, im, target_size=600, max_size=1000) -> (scores [R,C], pred_boxes [R,4C]) as numpy
    detect_persons(net, im, person_id, thresh=0.3, prop_dets=None) -> [N,5] (x1, y1, x2, y2, score) as numpy
    detect_persons_clip(net, frames [T,H,W,3], person_id, ...) -> T arrays [n_t,5]: detect_persons for every frame of a clip with the
        frame steps enqueued back to back (net.detect_enqueue) and ONE device -> host copy; = clip_finish(clip_enqueue(...))

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
from .proposal import RPN_DEFAULTS

SELECT_MAX_BOXES = 1024                          # ft_detect_select_fwd: detector rows + extra boxes of one frame

__all__ = ["PIXEL_MEANS", "blob_size", "stage_frame", "im_detect", "detect_persons", "detect_persons_clip", "clip_enqueue", "clip_finish", "clip_pack", "clip_unpack"]

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


class ClipHandle:
    """What clip_enqueue leaves on the device: dets [T,cap,5], counts [T], and everything the enqueued work still reads."""

    def __init__(self, dets, counts, keep):
        self.dets, self.counts, self._keep = dets, counts, keep


def _clip_extras(prop_dets, T: int, device):
    """prop_dets -> (extra fp32 [T,M,5] on the device, counts int32 [T] on the device) or (None, None).  A list of per-frame [m_t,5]
    arrays (None / empty allowed) is padded to the longest; a [T,M,5] array or tensor is taken whole."""
    if prop_dets is None:
        return None, None
    if isinstance(prop_dets, torch.Tensor):
        if prop_dets.dim() != 3 or prop_dets.shape[0] != T or prop_dets.shape[2] != 5:
            raise FlowtrackHipError(f"detect_persons_clip prop_dets: expected [T,M,5], got {tuple(prop_dets.shape)}")
        extra = prop_dets.to(device=device, dtype=torch.float32).contiguous()
        return extra, torch.full((T,), extra.shape[1], dtype=torch.int32, device=device)
    per = [np.zeros((0, 5), np.float32) if p is None else np.asarray(p, dtype=np.float32).reshape(-1, 5) for p in prop_dets]
    if len(per) != T:
        raise FlowtrackHipError(f"detect_persons_clip prop_dets: {len(per)} entries for {T} frames")
    M = max((len(p) for p in per), default=0)
    host = np.zeros((T, M, 5), dtype=np.float32)
    for t, p in enumerate(per):
        host[t, :len(p)] = p
    return torch.from_numpy(host).to(device), torch.from_numpy(np.array([len(p) for p in per], dtype=np.int32)).to(device)


def clip_enqueue(net, frames, person_id: int, thresh: float = 0.3, min_score: float = 0.0, prop_dets=None, target_size: int = TEST_SCALE,
                 max_size: int = TEST_MAX_SIZE, cap=None) -> ClipHandle:
    """Enqueues detect_persons for every frame of `frames` ([T,H,W,3] BGR uint8, numpy or tensor): one trunk plan (all frames share the
    blob shape), each frame staged by ft_detect_blob_fwd directly ahead of its replay, net.detect_enqueue into the frame's slot of
    dets [T,cap,5] / counts [T].  Nothing is read from the device (with frames and prop_dets already there, nothing crosses the bus);
    the first call at a blob shape builds and captures the two plans, which waits.  prop_dets: per-frame extra boxes, a list of
    [m_t,5] arrays or a [T,M,5] array / tensor.  cap: rows per frame, default post_nms_topN + M (every candidate can survive)."""
    net.eval()
    device = next(net.parameters()).device
    t = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or min(t.shape[1:3]) < 1:
        raise FlowtrackHipError("detect_persons_clip: expected BGR uint8 frames [T,H,W,3]")
    t = t.to(device).contiguous()
    T, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    extra, extra_counts = _clip_extras(prop_dets, T, device)
    M = 0 if extra is None else int(extra.shape[1])
    rows = max(RPN_DEFAULTS["TEST"][1] if net.rpn_post_nms_topN is None else int(net.rpn_post_nms_topN), 1)
    if rows + M > SELECT_MAX_BOXES:
        raise FlowtrackHipError(f"detect_persons_clip: {rows} detector rows + {M} extra boxes, ft_detect_select_fwd takes {SELECT_MAX_BOXES}")
    cap = rows + M if cap is None else int(cap)
    if cap < 1:
        raise FlowtrackHipError("detect_persons_clip: cap >= 1")
    dets = torch.zeros((T, cap, 5), dtype=torch.float32, device=device)
    counts = torch.zeros(T, dtype=torch.int32, device=device)
    if T == 0:
        return ClipHandle(dets, counts, ())
    im_scale, Hb, Wb = blob_size(H, W, target_size, max_size)
    if Hb < 1 or Wb < 1:
        raise FlowtrackHipError(f"detect_persons_clip: a {H}x{W} frame at scale {im_scale} leaves no blob")
    plan = net.trunk_plan(Hb, Wb)
    im_info = np.array([Hb, Wb, im_scale], dtype=np.float32)
    lib, means = _lib.load(), (ctypes.c_double * 3)(*PIXEL_MEANS)
    for i in range(T):
        with torch.cuda.device(device):
            check(lib.ft_detect_blob_fwd(t[i].data_ptr(), H, W, means, Hb, Wb, 1.0 / im_scale, 1.0 / im_scale, plan.x_static.data_ptr(),
                                         current_stream_handle(device)), "ft_detect_blob_fwd")
        net.detect_enqueue(plan, im_info, (H, W), (dets[i], counts[i:i + 1]), person_id, thresh, min_score,
                           extra[i] if M else None, extra_counts[i:i + 1] if M else None)
    return ClipHandle(dets, counts, (t, extra, extra_counts))


def clip_pack(handle: ClipHandle) -> torch.Tensor:
    """The handle's results as ONE device tensor of words, int32 [T, cap*5 + 1]: a frame's dets bits, then its count (what a
    multi-process caller gathers by rows before the download)."""
    T, cap = int(handle.dets.shape[0]), int(handle.dets.shape[1])
    return torch.cat((handle.dets.view(T, cap * 5).view(torch.int32), handle.counts.view(T, 1)), 1)


def clip_unpack(packed: np.ndarray):
    """clip_pack's rows on the host -> T arrays [n_t,5] float32."""
    packed = np.asarray(packed, dtype=np.int32)
    T, cap = packed.shape[0], (packed.shape[1] - 1) // 5
    rows = np.ascontiguousarray(packed[:, :cap * 5]).view(np.float32).reshape(T, cap, 5)
    return [rows[i, :min(max(int(packed[i, cap * 5]), 0), cap)].copy() for i in range(T)]


def clip_finish(handle: ClipHandle):
    """The clip's single device -> host copy: T arrays [n_t,5]."""
    if int(handle.dets.shape[0]) == 0:
        return []
    return clip_unpack(clip_pack(handle).cpu().numpy())


def detect_persons_clip(net, frames, person_id: int, thresh: float = 0.3, min_score: float = 0.0, prop_dets=None,
                        target_size: int = TEST_SCALE, max_size: int = TEST_MAX_SIZE, cap=None):
    """detect_persons over a clip: element t is bit for bit detect_persons(net, frames[t], person_id, thresh, prop_dets[t]) when
    min_score = 0 (a positive min_score drops candidates below it ahead of the NMS; cap below the survivor count keeps the first cap)."""
    return clip_finish(clip_enqueue(net, frames, person_id, thresh, min_score, prop_dets, target_size, max_size, cap))
