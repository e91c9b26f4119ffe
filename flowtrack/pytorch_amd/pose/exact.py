"""The exact-arg-max mode of the pose models (a mixin of host.PoseHost): key-point rows with the arg-max of the fp32 parity mode at
(mostly) fp16 speed.  The fp16 plan's heat maps are screened (ft_heatmap_argmax_screen), and only the crops the screen flags are
re-run in fp32.  `supports_exact` gates it: the screen's error bound was measured for the deconv head only.

Three ways in: forward_keypoint_rows_exact() reads the B flags on the host between the fp16 plan and the re-run; with nothing flagged
that read (a stream synchronisation per step) cost 10 % of the step.  exact_submit() / exact_finish() end the step on the device:
fp16 plan -> screen -> ft_gather_flagged_rows (flag compaction + copy of the flagged crops' INPUTS into a staging slot, all on the
device) -> an asynchronous copy of the small header {count, indices} to pinned memory -> event.  exact_finish(), called one step
later (or whenever the caller needs the rows), waits for that event — long past — and only if the count is non-zero runs the fp32
plan on the staged crops and patches their rows.  The caller's x may be overwritten as soon as exact_submit() returns.
exact_submit_plan() / exact_finish_plan() do the same with the device side recorded INSIDE the plan's graph (exact_in_plan)."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib
from ..engine import Plan
from ..hip_ops import FlowtrackHipError, check, current_stream_handle


class _ExactHandle:
    __slots__ = ("rows", "slot", "B", "H", "W", "done")


def _new_event() -> ctypes.c_void_p:
    ev = ctypes.c_void_p()
    check(_lib.load().ft_event_create(ctypes.byref(ev)), "ft_event_create")
    return ev


def _screen_state(B: int, H: int, W: int, device, **more) -> dict:
    """What one screened step of B crops keeps: the screen's flags and statistics, the staged inputs of the flagged crops, the
    header {count, indices} on the device and in pinned memory, the event behind the header copy, and whether a step is in flight."""
    return dict(flags=torch.empty(B, dtype=torch.int32, device=device), stats=torch.empty((B, 4), dtype=torch.float32, device=device),
                stage=torch.empty((B, 3, H, W), dtype=torch.float32, device=device), header=torch.zeros(1 + B, dtype=torch.int32, device=device),
                header_host=torch.zeros(1 + B, dtype=torch.int32).pin_memory(), event=None, busy=False, **more)


class ExactArgmax:
    #: forward_keypoint_rows_exact(): a crop is re-run in the fp32 parity arithmetic when ft_heatmap_argmax_screen flags it:
    #: E = exact_argmax_rel_bound x (range of the crop's fp16 heat maps) is taken as the bound of the fp16 mode's heat-map error,
    #: and a crop is flagged when two values of a map are closer than 2 E (an error of at most E per element cannot reorder
    #: values further apart), when a map's maximum is within E of 0 (the `score > 0` coordinate mask of max_preds could flip), or
    #: when anything is non-finite.  The bound is RELATIVE because the error follows the maps' range (the tests bound it as a
    #: fraction of the range); 1.6e-3 = 2 x the largest measured ratio (4.07e-3 on a range of 5.0 = 0.81e-3)
    exact_argmax_rel_bound: float = 1.6e-3

    def _check_exact_supported(self, what: str) -> None:
        if not self.supports_exact:
            raise FlowtrackHipError(f"{what}: the exact-arg-max mode is not available for {type(self).__name__} (its screen's error bound "
                                    "was measured for the deconv head only)")

    def _check_exact_allowed(self, what: str) -> None:
        """Entry check of the exact-arg-max mode: the model has the mode, and no flip test is set."""
        self._check_exact_supported(what)
        if self.flip_pairs is not None:
            raise FlowtrackHipError(f"{what}: flip_pairs is set, and the exact-arg-max mode does not combine with the flip test")

    def _exact_slots(self, B: int, H: int, W: int, device):
        """The two staging slots of exact_submit() for one input shape."""
        key = (B, H, W, str(device))
        st = self.__dict__.setdefault("_exact_state", {})
        ent = st.get(key)
        if ent is None:
            ent = st[key] = {"slots": [dict(_screen_state(B, H, W, device), event=_new_event()) for _ in range(2)], "next": 0}
        return ent

    def _record_exact_screen(self, prog, plan: Plan) -> None:
        """The mode's device side INSIDE the plan's graph: screen -> flag compaction + gather of the flagged crops' inputs -> header
        {count, indices} to pinned memory.  As graph nodes they cost their kernel time (~10 us); as five eager launches behind the
        replay they cost ~70 us of gaps per step.  exact_argmax_rel_bound is frozen into the plan, the event is made by the first
        exact_submit_plan()."""
        hm, x = plan.heatmaps, plan.x_static
        (B, _, H, W), (K, hh, hw) = x.shape, hm.shape[1:]
        ex = plan.exact = _screen_state(B, H, W, x.device, rel_bound=float(self.exact_argmax_rel_bound))
        prog.add("ft_heatmap_argmax_screen", hm.data_ptr(), B, K, hh, hw, ctypes.c_float(ex["rel_bound"]), ex["flags"].data_ptr(),
                 ex["stats"].data_ptr(), keep=(ex["flags"], ex["stats"]))
        prog.add("ft_gather_flagged_rows", ex["flags"].data_ptr(), B, x.data_ptr(), ctypes.c_longlong(3 * H * W * 4), ex["stage"].data_ptr(),
                 ex["header"].data_ptr(), keep=(ex["stage"], ex["header"]))
        prog.add("ft_memcpy_async", ex["header_host"].data_ptr(), ex["header"].data_ptr(), ctypes.c_size_t((1 + B) * 4), keep=(ex["header_host"],))

    def release_exact_state(self) -> None:
        """Destroy the events and drop the pinned headers / staging buffers of the asynchronous exact-arg-max paths (exact_submit
        slots and the per-plan state of exact_submit_plan).  Called when the plans are invalidated (weights, dtype or device changed)
        and by close(); a step that is still in flight is abandoned (its handle must not be finished afterwards)."""
        states = [sl for ent in self.__dict__.get("_exact_state", {}).values() for sl in ent["slots"]] + \
            [pl.exact for pl in self.__dict__.get("_plans", {}).values() if getattr(pl, "exact", None)]
        for st in states:
            if st["event"] is not None:
                _lib.load().ft_event_destroy(st["event"])
                st["event"], st["busy"] = None, False
        self.__dict__["_exact_state"] = {}

    @torch.no_grad()
    def exact_submit(self, x: torch.Tensor) -> _ExactHandle:
        """First half of the exact-arg-max step (see above): everything is queued on the current stream, nothing is waited for."""
        if self.keypoints_in_plan is None:
            raise FlowtrackHipError("set model.keypoints_in_plan = True / False (adjust_coords) before exact_submit()")
        self._check_exact_allowed("exact_submit")
        lib = _lib.load()
        B, _, H, W = x.shape
        if B > 1024:
            raise FlowtrackHipError("exact_submit: at most 1024 crops per call")
        ent = self._exact_slots(B, H, W, x.device)
        sl = ent["slots"][ent["next"]]
        if sl["busy"]:
            raise FlowtrackHipError("exact_submit: both staging slots are in flight: call exact_finish() on the older handle first")
        want = self.compute_dtype
        self.compute_dtype = torch.float16
        try:
            rows = self.forward_keypoint_rows(x).clone()
            hm = self._last_plan.heatmaps
        finally:
            self.compute_dtype = want
        sh = current_stream_handle(x.device)
        check(lib.ft_heatmap_argmax_screen(hm.data_ptr(), B, hm.shape[1], hm.shape[2], hm.shape[3], ctypes.c_float(self.exact_argmax_rel_bound),
                                           sl["flags"].data_ptr(), sl["stats"].data_ptr(), sh), "ft_heatmap_argmax_screen")
        xin = self._last_plan.x_static          # (fp32 NCHW: the plan's own copy of the batch)
        check(lib.ft_gather_flagged_rows(sl["flags"].data_ptr(), B, xin.data_ptr(), 3 * H * W * 4, sl["stage"].data_ptr(), sl["header"].data_ptr(), sh),
              "ft_gather_flagged_rows")
        check(lib.ft_memcpy_async(sl["header_host"].data_ptr(), sl["header"].data_ptr(), (1 + B) * 4, sh), "ft_memcpy_async")
        check(lib.ft_event_record(sl["event"], sh), "ft_event_record")
        sl["busy"] = True
        self._last_screen_stats = sl["stats"]
        h = _ExactHandle()
        h.rows, h.slot, h.B, h.H, h.W, h.done = rows, ent["next"], B, H, W, False
        ent["next"] ^= 1
        return h

    @torch.no_grad()
    def exact_finish(self, h: _ExactHandle):
        """Second half: (rows [B,K,3] with the parity mode's arg-max, number of crops re-run in fp32)."""
        if h.done:
            raise FlowtrackHipError("exact_finish: handle already finished")
        sl = self._exact_slots(h.B, h.H, h.W, h.rows.device)["slots"][h.slot]
        check(_lib.load().ft_event_synchronize(sl["event"]), "ft_event_synchronize")
        h.done = True
        try:
            n = self._rerun_staged(sl, h.rows, h.B, h.H, h.W)
        finally:
            sl["busy"] = False       # an exception inside the fp32 re-run must not pin the slot
        return h.rows, n

    @torch.no_grad()
    def exact_submit_plan(self, plan: Plan) -> Plan:
        """exact_submit() for a caller that owns the plan (plan_for(..., replica) with `exact_in_plan` set, its x_static filled in
        place): ONE graph replay — network, key-point rows, screen, gather, header copy — and an event.  The plan's buffers are the
        step's state, so a plan must be finished (exact_finish_plan) before it is submitted again: callers that keep several steps
        in flight rotate plan replicas."""
        self._check_exact_allowed("exact_submit_plan")
        ex = getattr(plan, "exact", None)
        if ex is None:
            raise FlowtrackHipError("exact_submit_plan: the plan was built without exact_in_plan (fp16, keypoints_in_plan, B <= 1024)")
        if ex["busy"]:
            raise FlowtrackHipError("exact_submit_plan: this plan's previous step was not finished")
        if ex["event"] is None:
            ex["event"] = _new_event()
        self.replay(plan)
        check(_lib.load().ft_event_record(ex["event"], current_stream_handle(plan.x_static.device)), "ft_event_record")
        ex["busy"] = True
        return plan

    @torch.no_grad()
    def exact_finish_plan(self, plan: Plan):
        """(plan.kp_rows with the flagged crops' rows replaced by the fp32 parity mode's, number of crops re-run)."""
        ex = plan.exact
        if not ex["busy"]:
            raise FlowtrackHipError("exact_finish_plan: nothing submitted")
        try:
            check(_lib.load().ft_event_synchronize(ex["event"]), "ft_event_synchronize")
            B, _, H, W = plan.x_static.shape
            n = self._rerun_staged(ex, plan.kp_rows, B, H, W)
        finally:
            ex["busy"] = False
        return plan.kp_rows, n

    def _rerun_staged(self, st: dict, rows, B: int, H: int, W: int) -> int:
        """A finished screened step: the n = header[0] flagged crops (inputs staged in st["stage"], indices in header[1:]) through
        the fp32 plan, their rows patched into `rows`.  Returns n."""
        hdr, stage = st["header_host"], st["stage"]
        n = int(hdr[0])
        if n:
            self._rerun_flagged(rows, hdr[1:1 + n].to(torch.int64).to(rows.device), lambda lo, hi: stage[lo:hi], B, H, W)
        return n

    def _rerun_flagged(self, rows, idx, crops, B: int, H: int, W: int) -> None:
        """The flagged crops of a batch of B (their indices in `idx`, int64 on the device; crops(lo, hi) = the inputs of idx[lo:hi])
        through the fp32 plan in buckets of 8 .. B crops; their rows patched into `rows`."""
        n = len(idx)
        want, ex_flag = self.compute_dtype, self.exact_in_plan
        self.compute_dtype, self.exact_in_plan = torch.float32, False
        try:
            lo = 0
            while lo < n:
                m = min(n - lo, B)
                bucket = next(b for b in (8, 16, 32, 64, 128, 256, 1 << 30) if b >= m or b >= B)
                bucket = min(bucket, max(B, 8))
                xb = self.static_input(bucket, H, W)
                take = min(m, bucket)
                xb[:take].copy_(crops(lo, lo + take))
                if take < bucket:
                    xb[take:].zero_()
                r32 = self.forward_keypoint_rows(xb)
                rows.index_copy_(0, idx[lo:lo + take], r32[:take])
                lo += take
        finally:
            self.compute_dtype, self.exact_in_plan = want, ex_flag

    @torch.no_grad()
    def forward_keypoint_rows_exact(self, x: torch.Tensor):
        """Key-point rows [B,K,3] with the arg-max of the fp32 parity mode at (mostly) fp16 speed — north_star's "keypoint
        argmax bit-exact vs CPU reference" for the fast mode (max_preds, lib/pose/utils/evaluation.py:11-20):
          1. the fp16 plan (heat maps + rows, as forward_keypoint_rows);
          2. ft_heatmap_argmax_screen: per crop a flag (see exact_argmax_rel_bound) and its statistics;
          3. flagged crops go through the fp32 plan (buckets of 8 .. B crops), their rows replace the fp16 ones.
        A crop that is not flagged has every top-1 / top-2 margin above twice the error bound and every maximum further than the
        bound from 0, so neither its arg-max nor its coordinate mask can differ from fp32's (its score and the +-0.25 px nudge
        come from the fp16 map).  What this costs depends on the heat maps: single-peak maps (a trained net) flag next to
        nothing, noise-like maps (random weights) nearly every crop — then the mode runs at fp32 speed.  Returns (rows [B,K,3]
        on the device — a buffer of this call, not the plan's —, number of crops re-run).  One device -> host read of B flags
        per call sits between 2 and 3."""
        if self.keypoints_in_plan is None:
            raise FlowtrackHipError("set model.keypoints_in_plan = True / False (adjust_coords) before forward_keypoint_rows_exact()")
        self._check_exact_allowed("forward_keypoint_rows_exact")
        want = self.compute_dtype
        if want not in (None, torch.float16) and next(self.parameters()).dtype != torch.float16:
            raise FlowtrackHipError("forward_keypoint_rows_exact() is the fp16 mode's exact-arg-max path: compute_dtype must be fp16")
        B = x.shape[0]
        self.compute_dtype = torch.float16
        try:
            rows = self.forward_keypoint_rows(x).clone()
            hm = self._last_plan.heatmaps
            flags = torch.empty(B, dtype=torch.int32, device=x.device)
            stats = torch.empty((B, 4), dtype=torch.float32, device=x.device)
            check(_lib.load().ft_heatmap_argmax_screen(hm.data_ptr(), B, hm.shape[1], hm.shape[2], hm.shape[3],
                                                       ctypes.c_float(self.exact_argmax_rel_bound), flags.data_ptr(), stats.data_ptr(),
                                                       current_stream_handle(x.device)), "ft_heatmap_argmax_screen")
            self._last_screen_stats = stats
            todo = torch.nonzero(flags.cpu()).flatten().to(x.device)
            self._rerun_flagged(rows, todo, lambda lo, hi: x.index_select(0, todo[lo:hi]), B, x.shape[2], x.shape[3])
        finally:
            self.compute_dtype = want
        return rows, len(todo)
