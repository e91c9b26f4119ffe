"""Numpy references of the device tracking pass (csrc/track_ops.hip, tracking/device_pass.py): nothing here is new arithmetic,
every function only arranges calls of the host functions the kernels restate, so that a test can compare bit for bit."""
import numpy as np

from flowtrack.pytorch_amd.tracking.flow_utils import box_propagation, nms
from flowtrack.pytorch_amd.tracking.net_utils import boxes_to_center_scale, heatmap_rows_to_image
from flowtrack.pytorch_amd.tracking.tracker import propagate_keypoints


def history_step(prev_hist, kps_prev, flow):
    """hist[t] [A,cap,K,2] float64 from hist[t-1], the previous frame's key points [n,K,3] and the flow t-1 -> t (None: a frame
    without flow, the history ages unmoved): [0] = the previous poses moved, [a] = hist[t-1][a-1] advanced by the same rule."""
    A, cap, K, _ = prev_hist.shape
    cur = np.zeros_like(prev_hist)
    if flow is None:
        cur[1:] = prev_hist[:-1]
        return cur
    kp = np.zeros((cap, K, 3), dtype=np.float64)
    kp[:len(kps_prev)] = kps_prev
    cur[0] = propagate_keypoints(kp, flow)[..., :2]
    for a in range(1, A):
        cur[a] = propagate_keypoints(prev_hist[a - 1], flow)
    return cur


def history_from_flows(kps_frames, flows, max_age, cap):
    """The moved-pose history [T,max_age+1,cap,K,2] of a clip on the CPU.  kps_frames[t]: [n_t,K,3]; flows[t-1]: [2,H,W]; a frame
    has a flow when its predecessor holds at least one pose (tools/tracking/demo.py: tracking_pass_steps)."""
    T, K = len(kps_frames), np.asarray(kps_frames[0]).shape[1]
    hist = np.zeros((T, max_age + 1, cap, K, 2), dtype=np.float64)
    for t in range(1, T):
        flow = np.asarray(flows[t - 1]) if len(kps_frames[t - 1]) else None
        hist[t] = history_step(hist[t - 1], np.asarray(kps_frames[t - 1], dtype=np.float64), flow)
    return hist


def propagate_ref(kps_prev, flow, older):
    """ft_track_propagate: (moved [1+n_old,P,K,2] float64, boxes [P,4] float32)."""
    moved = [propagate_keypoints(kps_prev, flow)[..., :2]] + [propagate_keypoints(o, flow) for o in older]
    return np.stack(moved), box_propagation(kps_prev, flow).astype(np.float32)


def select_ref(dets, kp_det, prop_boxes, prev_boxes, M, thresh, max_keep, rh, rw, bucket, K):
    """ft_track_select: lines 118-133 of tools/tracking/demo.py + what PoseRunner.submit makes of the propagated boxes."""
    cur = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    n = len(cur)
    src = np.arange(n)
    if M > 0:
        prop_dets = np.concatenate((prop_boxes[:M], prev_boxes[:M, 4:5]), axis=1).astype(np.float32)
        allb = np.concatenate((cur, prop_dets), 0)
        with np.errstate(all="ignore"):
            keep = nms(allb, thresh)
        keep = keep[:max_keep]
        cur, src = allb[keep], keep
    kps = np.zeros((len(cur), K, 3), dtype=np.float32)
    from_det = src < n
    kps[from_det] = np.asarray(kp_det, dtype=np.float32).reshape(-1, K, 3)[src[from_det]]
    slots = np.nonzero(~from_det)[0]
    params = np.zeros((bucket, 3), dtype=np.float32)
    if len(slots):
        centers, scales = boxes_to_center_scale(cur[slots, :4], (rh, rw))
        params[:len(slots), :2] = centers
        params[:len(slots), 2] = scales
        params[len(slots):] = params[0]
    else:
        params[:] = (0.0, 0.0, 1.0)
    return {"boxes": cur, "src": src.astype(np.int32), "count": len(cur), "kps": kps, "nprop": len(slots),
            "prop_slot": slots.astype(np.int32), "params": params}


def place_rows_ref(kps, rows, boxes, slots, hm_hw, rh, rw):
    """ft_track_place_rows: kps with the rows of `slots` replaced by heatmap_rows_to_image of rows[:len(slots)]."""
    out = kps.copy()
    if len(slots):
        centers, scales = boxes_to_center_scale(boxes[slots, :4], (rh, rw))
        out[slots] = heatmap_rows_to_image(rows[:len(slots)], centers, scales, hm_hw)
    return out
