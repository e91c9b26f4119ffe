"""What every pose model shares, and nothing of any trunk: the plan cache, forward / forward_flip / replay, the flip test and the key
points inside the plan, the exact-arg-max mode (exact.ExactArgmax), initialisation.  A model family (resnet_models, densenet,
hourglass) supplies its parameters, _check_input_size and the one hook _record_net."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from ..engine import HipModule, Plan
from ..hip_ops import ActView, FlowtrackHipError, Program, new_act, new_rowpacked_act, record_maxpool, record_pack_input, record_scale_shift_act
from ..params import BatchNormParams, ConvParams
from .exact import ExactArgmax


class _Stages(dict):
    """plan.stages: the activation view behind each stage.  A stage whose last block was recorded in the exit form
    (PoseResnet.fuse_stage_exit) may never write its full map: it has no entry, and asking for it says why."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.absent = {}

    def __missing__(self, key):
        if key in self.absent:
            raise FlowtrackHipError(f"plan.stages[{key!r}]: {self.absent[key]}")
        raise KeyError(key)


class PoseHost(ExactArgmax, HipModule):
    """The plan machinery of a pose model: num_classes heat maps [B,K,h,w] fp32 from crops [B,3,H,W], whatever network is in
    between (_record_net)."""
    #: the exact-arg-max mode (exact_in_plan, exact_submit*, forward_keypoint_rows_exact): its error bound was measured for the deconv head
    supports_exact: bool = False
    #: None: plans end at the heatmaps (the reference's forward).  True / False: plans also run max_preds on the heatmaps
    #: (with / without the adjust_coords nudge, lib/pose/utils/evaluation.py:11-35) and forward_keypoints() returns them
    keypoints_in_plan = None
    #: record the exact-arg-max mode's screen + flagged-crop gather inside fp16 plans (needs keypoints_in_plan); see exact_submit_plan
    exact_in_plan: bool = False
    #: None: no flip test.  A sequence of (a, b) left/right joint pairs (tools/pose/main.get_flip_pairs; () = mirror and average, no swap):
    #: forward_flip(), plan_for() and, with keypoints_in_plan set, forward_keypoints() / forward_keypoint_rows() use the FLIP PLAN of a
    #: shape: the ordinary launch list at batch 2B between ft_hflip_nchw_f32 (x[:B] mirrored into x[B:]) and ft_heatmap_flip_merge
    #: (the two halves averaged, left/right joints swapped back, and the key points of the merged maps).  forward() never reads it
    flip_pairs = None
    #: init_weights(): the keyword arguments of the convs' kaiming_normal_, and whether their biases are zeroed
    kaiming_args = dict(mode="fan_out", nonlinearity="relu")
    zero_conv_bias: bool = False

    # -- initialisation / loading ---------------------------------------------------------------
    @classmethod
    def rewrite_checkpoint_keys(cls, state_dict: dict) -> dict:
        """A pretrained backbone's keys under this model's parameter names: here they are the same."""
        return state_dict

    def init_weights(self, pretrained: str = "") -> None:
        """The reference's init_weights (resnet.py:38-49, densenet.py:122-148, hourglass.py:166-173): the checkpoint at `pretrained`
        where there is one, else every conv kaiming_normal_(**kaiming_args) and every BatchNorm (1, 0)."""
        if pretrained and os.path.isfile(pretrained):
            print("=> loading pretrained model {}".format(pretrained))
            self.load_state_dict(self.rewrite_checkpoint_keys(torch.load(pretrained, map_location="cpu")), strict=False)
            return
        for m in self.modules():
            if isinstance(m, ConvParams):
                nn.init.kaiming_normal_(m.weight, **self.kaiming_args)
                if self.zero_conv_bias and m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, BatchNormParams):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._invalidate()

    def _init_head(self) -> None:
        """The part of the reference's init_net behind init_weights (a head's own initialisation); none by default."""

    def init_net(self, pretrained: str = "") -> None:
        self.init_weights(pretrained)
        self._init_head()
        self._invalidate()

    def _invalidate(self):
        self.release_exact_state()
        super()._invalidate()

    def close(self) -> None:
        """Release what the module holds outside torch's allocator (events of the exact-arg-max paths) and its captured plans."""
        self._invalidate()

    # -- plan construction ----------------------------------------------------------------------
    def _flip_perm(self):
        """flip_pairs as the channel permutation of ft_heatmap_flip_merge (merged map k reads map perm[k] of the mirrored pass), validated
        as tools/pose/main._flip_back validates its pairs; None when flip_pairs is None."""
        if self.flip_pairs is None:
            return None
        if self.exact_in_plan:
            raise FlowtrackHipError("flip_pairs is set: the exact-arg-max mode (exact_in_plan) does not combine with the flip test")
        perm, seen = list(range(self.num_classes)), set()
        try:
            pairs = [(int(a), int(b)) for a, b in self.flip_pairs]
        except (TypeError, ValueError):
            raise FlowtrackHipError(f"flip_pairs must be None or a sequence of (a, b) joint pairs, got {self.flip_pairs!r}")
        for a, b in pairs:
            if not (0 <= a < self.num_classes and 0 <= b < self.num_classes):
                raise FlowtrackHipError(f"flip pair ({a}, {b}) does not fit {self.num_classes} heatmap channels: wrong dataset table?")
            if a in seen or b in seen:
                raise FlowtrackHipError(f"flip pair ({a}, {b}): a joint may appear in one pair only")
            seen.update((a, b))
            perm[a], perm[b] = b, a
        return tuple(perm)

    def _check_input_size(self, H: int, W: int) -> None:
        """Raise FlowtrackHipError where the network does not take an H x W input."""
        raise NotImplementedError

    def _record_net(self, prog, x_static, dtype, device):
        """Record everything between "the input is staged in x_static [B,3,H,W] fp32" and "the heat maps exist": returns (stages,
        the NCHW fp32 heat maps the plan's tail reads).  The one hook a model family must supply."""
        raise NotImplementedError

    def _keypoint_buffers(self, plan: Plan, B: int, device) -> None:
        """The key points of a plan, written as (x, y, score) rows — what the tracking glue and the multi-GPU gather consume; scores /
        coords are views.  None where keypoints_in_plan is None."""
        plan.kp_idx = plan.kp_rows = None
        if self.keypoints_in_plan is not None:
            plan.kp_idx = torch.empty((B, self.num_classes), dtype=torch.int32, device=device)
            plan.kp_rows = torch.empty((B, self.num_classes, 3), dtype=torch.float32, device=device)
            plan.kp_score, plan.kp_coords = plan.kp_rows[:, :, 2:], plan.kp_rows[:, :, :2]

    def _build_plan(self, B: int, H: int, W: int, device, dtype, perm=None) -> Plan:
        """The plan of one input shape: the staged input (and its mirrored half in a flip plan), the network's own launches
        (_record_net: what a model family supplies), then the flip merge / the key points / the exact-arg-max screen."""
        self._check_input_size(H, W)
        prog = Program(self._side_stream(device))
        B0 = B
        if perm is not None:
            # flip plan: everything below is the ordinary launch list at batch 2B; crops [B0, 2 B0) are the mirrored copies of [0, B0)
            B = 2 * B0
        x_static = torch.empty((B, 3, H, W), dtype=torch.float32, device=device)
        if perm is not None:
            prog.add("ft_hflip_nchw_f32", x_static.data_ptr(), x_static[B0:].data_ptr(), B0, 3, H, W)
        stages, heatmaps = self._record_net(prog, x_static, dtype, device)
        K, hh, hw = self.num_classes, heatmaps.shape[2], heatmaps.shape[3]
        if perm is not None:
            # last launch: average the two halves (mirror + left/right swap of the second) and, with keypoints_in_plan, the key points
            # of the merged maps — in place of the separate ft_heatmap_keypoint_rows launch
            merged = torch.empty((B0, K, hh, hw), dtype=torch.float32, device=device)
            plan = Plan(prog, x_static=x_static[:B0], heatmaps=merged)
            plan.stages, plan.heatmaps_raw, plan.x_full = stages, heatmaps, x_static
            plan.flip_perm = torch.tensor(perm, dtype=torch.int32, device=device)
            self._keypoint_buffers(plan, B0, device)
            keep = [merged, heatmaps, plan.flip_perm] + ([plan.kp_idx, plan.kp_rows] if plan.kp_idx is not None else [])
            prog.add("ft_heatmap_flip_merge", heatmaps.data_ptr(), heatmaps[B0:].data_ptr(), plan.flip_perm.data_ptr(), B0, K, hh, hw,
                     int(bool(self.keypoints_in_plan)), merged.data_ptr(), plan.kp_idx.data_ptr() if plan.kp_idx is not None else None,
                     plan.kp_rows.data_ptr() if plan.kp_rows is not None else None, keep=tuple(keep))
            return plan
        plan = Plan(prog, x_static=x_static, heatmaps=heatmaps)
        plan.stages = stages
        if self.keypoints_in_plan is not None:
            # max_preds (+ the 0.25 px nudge of final_preds) as the last launch of the plan: no extra stream work per call
            self._keypoint_buffers(plan, B, device)
            prog.add("ft_heatmap_keypoint_rows", heatmaps.data_ptr(), B, K, hh, hw, int(bool(self.keypoints_in_plan)),
                     plan.kp_idx.data_ptr(), plan.kp_rows.data_ptr(), keep=(plan.kp_idx, plan.kp_rows))
            if self.exact_in_plan and dtype == torch.float16 and B <= 1024:
                self._record_exact_screen(prog, plan)
        return plan

    def plan_for(self, B: int, H: int, W: int, replica: int = 0) -> Plan:
        """The plan (launch list + activation buffers + graph) of one input shape.  `replica` > 0 gives an independent copy
        with its own buffers — same packed weights, same tile picks — for callers that keep several batches of one shape
        in flight on different streams (tracking.PoseRunner per clip, tools/tracking/demo.run_clips)."""
        return self._plan_for(B, H, W, replica, self._flip_perm())

    def _plan_for(self, B: int, H: int, W: int, replica: int = 0, perm=None) -> Plan:
        """plan_for() with the flip test stated by the caller: perm = None is the plain plan of the shape whatever flip_pairs says."""
        if self.exact_in_plan:
            self._check_exact_supported("exact_in_plan")
        device, dtype = self._resolve()
        key = (B, H, W, device, dtype, self.keypoints_in_plan) + (("exact", float(self.exact_argmax_rel_bound)) if self.exact_in_plan else ()) + \
            ((replica,) if replica else ()) + ((("flip",) + tuple(perm),) if perm is not None else ())
        return self._cached_plan(key, lambda: self._build_plan(B, H, W, device, dtype, perm))

    def static_input(self, B: int, H: int, W: int) -> torch.Tensor:
        """The plan's own input buffer [B,3,H,W] fp32 (the fixed address its graph reads).  A producer that writes its
        batch here and passes this tensor to forward() skips the 38 MB staging copy per call (zero-copy binding)."""
        return self.plan_for(B, H, W).x_static

    @torch.no_grad()
    def forward(self, x: torch.Tensor, copy_output: bool = True) -> torch.Tensor:
        """x: [B,3,H,W] on the model's GPU -> heatmaps [B,K,H/4,W/4] fp32 (pose_deconv.py:32-46)."""
        return self._forward(x, copy_output, None)

    @torch.no_grad()
    def forward_flip(self, x: torch.Tensor, copy_output: bool = True) -> torch.Tensor:
        """The flip test of the reference (tools/pose/main.py:289-299) as ONE plan: x and its mirror image through the net as a batch
        of 2B, then (heatmaps(x) + heatmaps(mirrored x) mirrored back with the `flip_pairs` channels swapped) * 0.5 -> [B,K,H/4,W/4]
        fp32.  flip_pairs must be set; () mirrors and averages without a swap."""
        perm = self._flip_perm()
        if perm is None:
            raise FlowtrackHipError("set model.flip_pairs (tools/pose/main.get_flip_pairs; () = no left/right swap) before forward_flip()")
        return self._forward(x, copy_output, perm)

    def _forward(self, x: torch.Tensor, copy_output: bool, perm) -> torch.Tensor:
        self._check_eval()
        if x.dim() != 4 or x.shape[1] != 3:
            raise FlowtrackHipError(f"expected [B,3,H,W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        plan = self._plan_for(B, H, W, 0, perm)
        if x.device != plan.x_static.device:
            raise FlowtrackHipError("input and model are on different devices")
        if x.data_ptr() != plan.x_static.data_ptr():   # zero-copy when the caller filled static_input() in place
            plan.x_static.copy_(x)  # dtype cast + staging into the graph's fixed input address
        self.run(plan)
        self._last_plan = plan
        return plan.heatmaps.clone() if copy_output else plan.heatmaps

    @torch.no_grad()
    def replay(self, plan: Plan) -> Plan:
        """Run a plan whose static input the caller filled in place (plan_for(...).x_static): forward() without the second
        plan look-up and the shape checks — the per-call host cost matters to the tracking pass, one small batch per frame."""
        self._check_eval()
        self.run(plan)
        self._last_plan = plan
        return plan

    @torch.no_grad()
    def forward_keypoints(self, x: torch.Tensor):
        """forward() with max_preds inside the plan (set `keypoints_in_plan` first): returns the plan's static buffers
        (heatmaps [B,K,h,w], idx int32 [B,K], scores [B,K,1], coords [B,K,2] in heatmap pixels), valid until the next call."""
        if self.keypoints_in_plan is None:
            raise FlowtrackHipError("set model.keypoints_in_plan = True / False (adjust_coords) before forward_keypoints()")
        hm = self._forward(x, False, self._flip_perm())      # (with flip_pairs set: the merged maps and their key points)
        plan = self._last_plan
        return hm, plan.kp_idx, plan.kp_score, plan.kp_coords

    @torch.no_grad()
    def forward_keypoint_rows(self, x: torch.Tensor) -> torch.Tensor:
        """forward_keypoints() returning only the plan's [B,K,3] (x, y, score) rows in heatmap pixels (static buffer, valid
        until the next call): the form `lib/tracking/net_utils.py` concatenates preds and maxvals into."""
        self.forward_keypoints(x)
        return self._last_plan.kp_rows


class PooledStem:
    """The 7x7 / s2 / p3 stem conv + BatchNorm + ReLU + 3x3 / s2 max-pool in front of the ResNet and DenseNet trunks, and its two
    switches (a mixin of PoseHost subclasses)."""
    #: the stem's max-pool inside the stem conv launch (ft_conv_desc.pool); FT_FUSE_STEM_POOL=0 keeps the two launches
    fuse_stem_pool: bool = os.environ.get("FT_FUSE_STEM_POOL", "1") != "0"
    #: the fused stem reads the NCHW fp32 input itself (ft_conv_desc.x_nchw_f32): no pack launch, no packed copy, bit-identical
    #: results; FT_FUSE_STEM_PACK=0 keeps ft_pack_nchw_to_nhwc in front of it.  Batch 64 x 256x192, same box: pack 18.7 us + stem 38.5
    #: us -> stem 46.2 us, 59.52 / 59.31 -> 59.71 / 59.61 k crops/s (the first version, predicated global loads instead of
    #: out-of-range buffer loads, ran the stem at 66 us: every load in its own divergent region behind a full wait)
    fuse_stem_pack: bool = os.environ.get("FT_FUSE_STEM_PACK", "1") != "0"

    def _stem_pools(self, dtype) -> bool:
        return self.fuse_stem_pool and dtype == torch.float16

    def record_stem(self, prog, label: str, pool_label: str, conv, bn, x_static, out: ActView, dtype, device, copy_label: str = ""):
        """Stage the stem's input and return record(lo, hi), which records the stem of crops [lo, hi) of x_static [B,3,H,W] into the
        same crops of `out` [B, H/4, W/4, conv.cout].  One kernel row = one K-run.  fp16: conv + bn + relu + max-pool are ONE launch
        (ft_conv_desc.pool; its patch starts one stem column further left: 5 physical pad columns instead of 3), the [B, H/2, W/2,
        cout] stem map never exists, and with fuse_stem_pack the launch gathers its patches from x_static (the packed buffer is
        geometry only).  Otherwise: pack, conv, max-pool, whole batch only; `copy_label` names the identity affine that carries the
        pooled map into `out` where `out` is a channel window (the max-pool kernel writes dense buffers: x * 1 + 0, exactly)."""
        B, _, H, W = x_static.shape
        pool_in_stem = self._stem_pools(dtype)
        planar_in = pool_in_stem and self.fuse_stem_pack
        a_in = new_rowpacked_act(B, H, W, 3, 5 if pool_in_stem else 3, dtype, "meta" if planar_in else device)
        if not planar_in:
            record_pack_input(prog, x_static, a_in)
        stem = self.fused(label + (pool_label if pool_in_stem else ""), conv.weight, stride=2, pad=3, bn=bn.as_dict(), act="relu",
                          dtype=dtype, device=device)

        def record(lo: int = 0, hi: int = B) -> None:
            if pool_in_stem:
                stem.record(prog, a_in.batch_slice(lo, hi), out.batch_slice(lo, hi), pool=True, x_nchw=x_static[lo:hi] if planar_in else None)
                return
            a1 = new_act(B, H // 2, W // 2, conv.cout, dtype, device)
            stem.record(prog, a_in, a1)
            pooled = new_act(B, H // 4, W // 4, conv.cout, dtype, device) if copy_label else out
            record_maxpool(prog, a1, pooled)
            if copy_label:
                ident = self._cached(copy_label, dtype, device, lambda: (torch.ones(conv.cout, dtype=torch.float32, device=device),
                                                                         torch.zeros(conv.cout, dtype=torch.float32, device=device)))
                record_scale_shift_act(prog, pooled, out, ident[0], ident[1], None)
        return record
