"""The clip's sequential tracking pass with the host out of the GPU's critical path (tools/tracking/demo.py: tracking_pass_steps
is the host form: per frame it reads the flow field, runs box_propagation + nms in numpy, fills a pinned parameter buffer,
launches crop + plan, waits for the rows, and only then starts the next frame).

Here every frame of the clip is enqueued at once, five launches per frame on one stream and no host wait between them:
ft_track_propagate (previous poses and the moved-pose history advanced by the flow, propagated boxes) -> ft_track_select (union
with the detector boxes, box NMS, cap, crop parameters into a device buffer) -> ft_crop_affine_fwd (reads those parameters,
writes the pose plan's input) -> the plan's graph -> ft_track_place_rows (the plan's rows into image pixels, into the frame's
key points).  What depends on earlier frames (how many boxes survived, how many of them are propagated ones) stays in device
int32 words; what the host must know to enqueue (buffer sizes, the plan bucket) follows from the detector counts and
`max_boxes` alone, which is why the pass requires that bound.  The kernels restate the host functions bit for bit
(csrc/track_ops.hip), so the boxes and key points are the host pass's, given the same pose rows.

The track ids are host bookkeeping that nothing on the device waits for: they are assigned afterwards from ONE download (boxes,
counts, key points, moved-pose history) by HistoryTracker, which reads a track's propagated pose from the history instead of
moving it by a flow field.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from .._lib import check
from ..hip_ops import current_stream_handle
from .net_utils import PoseRunner
from .tracker import HistoryTracker

MAX_UNION = 512                                          # ft_track_select: detector boxes + the previous frame's cap


def _carve(sections, buf_of):
    """[(name, torch dtype, shape)] laid out in one byte buffer buf_of(nbytes), every section 16-byte aligned
    -> (the buffer, name -> its typed view)."""
    spans, total = {}, 0
    for name, dtype, shape in sections:
        total = -(-total // 16) * 16
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        spans[name] = (total, nbytes)
        total += nbytes
    buf = buf_of(-(-total // 16) * 16)
    return buf, {name: buf[spans[name][0]:spans[name][0] + spans[name][1]].view(dtype).view(shape) for name, dtype, shape in sections}


class DeviceTrackingPass:
    """run() = tools/tracking/demo.tracking_pass for one clip whose frames, flows and detector key points are on the GPU."""

    def __init__(self, pose_net, inp_res=(256, 192), max_age: int = 1):
        """max_age: FlowTracker's (frames a track survives without a match = the depth of the moved-pose history).  Every
        launch of run() goes to torch's current stream."""
        self.net, self.inp_res, self.max_age = pose_net, tuple(inp_res), int(max_age)
        self.runner = None                                 # built on the first run(): the constructor touches no device
        self.last_timing = {}                              # run(): seconds spent enqueuing, waiting for the download, assigning ids

    def schedule(self, dets, max_boxes):
        """What the host knows of every frame before anything runs, from the detector counts alone: per frame a dict with
        n (detector boxes), cap (boxes kept at most), prev_cap, bucket (pose plan batch of the propagated boxes) and has_prev
        (the previous frame holds at least one pose: it does as soon as any frame so far had a detector box, because box NMS
        never empties a union).  Raises ValueError for what the device pass cannot run."""
        if max_boxes is None:
            raise ValueError("DeviceTrackingPass needs max_boxes (an int or '2x'): without a bound on the boxes kept per frame "
                             "no buffer size or plan bucket is known before the clip runs; the uncapped pass is the host's "
                             "(tools/tracking/demo.tracking_pass)")
        if max_boxes != "2x" and int(max_boxes) < 1:
            raise ValueError(f"max_boxes = {max_boxes!r}: at least 1")
        frames, prev_cap, has_prev = [], 0, False
        for t, d in enumerate(dets):
            n = len(np.asarray(d).reshape(-1, 5))
            cap = max(2 * n, 4) if max_boxes == "2x" else int(max_boxes)
            if n > cap:
                raise ValueError(f"frame {t}: {n} detector boxes exceed the cap of {cap} (max_boxes = {max_boxes!r})")
            bucket = PoseRunner.BUCKETS[0]
            if has_prev:
                if n + prev_cap > MAX_UNION:
                    raise ValueError(f"frame {t}: {n} detector boxes + {prev_cap} boxes the previous frame may hold exceed the "
                                     f"{MAX_UNION} boxes of the device NMS")
                bucket = next((b for b in PoseRunner.BUCKETS if b >= min(cap, prev_cap)), None)
                if bucket is None:
                    raise ValueError(f"frame {t}: up to {min(cap, prev_cap)} propagated boxes exceed the largest pose plan "
                                     f"({PoseRunner.BUCKETS[-1]} crops)")
            frames.append({"n": n, "cap": cap, "prev_cap": prev_cap, "bucket": bucket, "has_prev": has_prev})
            has_prev = has_prev or n > 0
            prev_cap = cap
        return frames

    def run(self, frames_dev, dets, kp_det, flows_dev, thresh: float = 0.3, max_boxes=None):
        """frames_dev: uint8 [T,H,W,3] on the GPU; dets[t]: [n_t,5] detector boxes (host); kp_det: their key points, a device
        tensor [T,>=max n_t,K,3] or a per-frame list of [n_t,K,3] arrays; flows_dev: float32 [T-1,2,H,W] on the GPU.
        Returns tracking_pass()'s per-frame list of {"boxes", "keypoints", "ids"}, each with "src" as well: per box its index
        into the frame's union (below n_t: a detector box, else a propagated one)."""
        t_start = time.perf_counter()
        sched = self.schedule(dets, max_boxes)
        T = len(sched)
        if T == 0:
            return []
        if self.runner is None:
            self.runner = PoseRunner(self.net, self.inp_res)
        r = self.runner
        dev, K, A = r.dev, r.K, self.max_age + 1
        if frames_dev.dtype != torch.uint8 or frames_dev.dim() != 4 or not frames_dev.is_contiguous() or len(frames_dev) != T:
            raise ValueError("frames must be one contiguous uint8 [T,H,W,C] device tensor, a frame per entry of dets")
        _, H, W, C = frames_dev.shape
        if T > 1 and (flows_dev.dtype != torch.float32 or tuple(flows_dev.shape) != (T - 1, 2, H, W) or not flows_dev.is_contiguous()):
            raise ValueError(f"flows must be a contiguous float32 [{T - 1},2,{H},{W}] device tensor")
        nmax = max(1, max(f["n"] for f in sched))
        capmax = max(f["cap"] for f in sched)
        bmax = max(f["bucket"] for f in sched)
        dets_host = np.zeros((T, nmax, 5), dtype=np.float32)
        for t, d in enumerate(dets):
            dets_host[t, :sched[t]["n"]] = np.asarray(d, dtype=np.float32).reshape(-1, 5)
        dets_dev = torch.from_numpy(dets_host).to(dev)
        if not torch.is_tensor(kp_det):
            kp_host = np.zeros((T, nmax, K, 3), dtype=np.float32)
            for t, k in enumerate(kp_det):
                kp_host[t, :sched[t]["n"]] = np.asarray(k, dtype=np.float32).reshape(-1, K, 3)
            kp_det = torch.from_numpy(kp_host)
        kp_det = kp_det.to(device=dev, dtype=torch.float32).contiguous()
        if kp_det.dim() != 4 or kp_det.shape[0] != T or kp_det.shape[1] < nmax or tuple(kp_det.shape[2:]) != (K, 3):
            raise ValueError(f"kp_det must be [{T},>={nmax},{K},3], got {tuple(kp_det.shape)}")
        # one zeroed arena: what the host reads afterwards first (one download), the per-frame scratch behind it
        results = [("hist", torch.float64, (T, A, capmax, K, 2)), ("boxes", torch.float32, (T, capmax, 5)),
                   ("kps", torch.float32, (T, capmax, K, 3)), ("src", torch.int32, (T, capmax)), ("count", torch.int32, (T,))]
        scratch = [("nprop", torch.int32, (T,)), ("prop_slot", torch.int32, (bmax,)), ("params", torch.float32, (bmax, 3)),
                   ("prop_boxes", torch.float32, (capmax, 4))]
        arena, v = _carve(results + scratch, lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev))
        ptr = {name: (ten.data_ptr(), ten[0].numel() * ten.element_size()) for name, ten in v.items()}
        at = lambda name, t: ptr[name][0] + t * ptr[name][1]                       # noqa: E731
        kp_stride, det_stride, frame_stride = kp_det[0].numel() * 4, nmax * 5 * 4, H * W * C
        flow_stride = 2 * H * W * 4
        lib, sh = r.lib, current_stream_handle(dev)
        rh, rw = self.inp_res
        for t, f in enumerate(sched):
            if not f["has_prev"]:
                if t > 0 and A > 1:                    # a frame without flow: the history ages unmoved
                    v["hist"][t, 1:].copy_(v["hist"][t - 1, :-1])
                if f["n"] == 0:
                    continue                           # nothing so far: the frame's count stays 0
                check(lib.ft_track_select(dets_dev.data_ptr() + t * det_stride, kp_det.data_ptr() + t * kp_stride, f["n"], None, None,
                                          0, None, K, thresh, f["cap"], f["cap"], rh, rw, f["bucket"], at("boxes", t), at("src", t),
                                          at("count", t), at("kps", t), at("nprop", t), ptr["prop_slot"][0], ptr["params"][0], sh),
                      "ft_track_select")
                continue
            check(lib.ft_track_propagate(at("kps", t - 1), flows_dev.data_ptr() + (t - 1) * flow_stride, H, W,
                                         at("hist", t - 1) if A > 1 else None, A - 1, capmax, K, at("hist", t),
                                         ptr["prop_boxes"][0], sh), "ft_track_propagate")
            check(lib.ft_track_select(dets_dev.data_ptr() + t * det_stride if f["n"] else None,
                                      kp_det.data_ptr() + t * kp_stride if f["n"] else None, f["n"], ptr["prop_boxes"][0],
                                      at("boxes", t - 1), f["prev_cap"], at("count", t - 1), K, thresh, f["cap"], f["cap"], rh, rw,
                                      f["bucket"], at("boxes", t), at("src", t), at("count", t), at("kps", t), at("nprop", t),
                                      ptr["prop_slot"][0], ptr["params"][0], sh), "ft_track_select")
            plan = r._plan(f["bucket"])
            r._crop(frames_dev.data_ptr() + t * frame_stride, H, W, C, ptr["params"][0], f["bucket"], plan.x_static.data_ptr(), sh)
            r._replay(plan, sh)
            hh, hw = plan.heatmaps.shape[2], plan.heatmaps.shape[3]
            check(lib.ft_track_place_rows(plan.kp_rows.data_ptr(), at("boxes", t), ptr["prop_slot"][0], at("nprop", t), f["bucket"],
                                          f["cap"], K, hh, hw, rh, rw, at("kps", t), sh), "ft_track_place_rows")
        # the one download: pinned memory behind an event
        nres = v["nprop"].data_ptr() - arena.data_ptr()
        host = torch.empty(nres, dtype=torch.uint8, pin_memory=True)
        host.copy_(arena[:nres], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        t_enqueued = time.perf_counter()
        done.synchronize()
        t_done = time.perf_counter()
        _, hv = _carve(results, lambda nbytes: host[:nbytes])
        hv = {name: ten.numpy() for name, ten in hv.items()}
        tracker = HistoryTracker(max_age=self.max_age)
        out = []
        for t, f in enumerate(sched):
            c = int(hv["count"][t])
            boxes, kps = hv["boxes"][t, :c].copy(), hv["kps"][t, :c].copy()
            ids = tracker.update(kps, boxes, hv["hist"][t] if f["has_prev"] else None)
            out.append({"boxes": boxes, "keypoints": kps, "ids": ids, "src": hv["src"][t, :c].copy()})
        self.last_timing = {"enqueue_s": t_enqueued - t_start, "wait_s": t_done - t_enqueued, "ids_s": time.perf_counter() - t_done}
        return out

    def close(self) -> None:
        if self.runner is not None:
            self.runner.close()
            self.runner = None
