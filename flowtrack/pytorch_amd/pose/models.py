"""Pose networks of FlowTrack on MI355X: ResNet-50/101/152 trunk + the 3x ConvTranspose(4,2,1) head, the FPN top-down head or the
lateral-deconv head, + 1x1 heatmap conv, executed as fused HIP launches (libflowtrack_hip.so).

Drop-in surface (reference: lib/pose/models/pose_deconv.py:12-63,166-179, pose_fpn.py:48-104,171-184, pose_net.py:30-91,163-177,
resnet.py:15-55, blocks.py:83-120):
    models.deconv(backbone: str, num_classes: int, pretrained: bool) -> module
    models.fpn(backbone: str, num_classes: int, pretrained: bool) -> module
    models.pose(backbone: str, num_classes: int, pretrained: bool) -> module
    models.hg(num_classes: int, num_stacks: int) -> module            (hourglass.py:227-231; forward returns one map per stack)
    module.forward(x[B,3,H,W]) -> heatmaps [B,K,H/4,W/4] (fp32)
    module.state_dict() / load_state_dict() / init_net(path) / .cuda() / .half() / .eval()
with the reference's parameter names and shapes, so its checkpoints
(`ckpt['state_dict']`, tools/pose/main.py:176-181) and torchvision-keyed ImageNet backbones
(`data/pretrained/<backbone>.pth`, loaded strict=False) load unchanged.

What differs by design: eval-mode BatchNorm and ReLU / the residual add are folded into each
conv's epilogue; activations live in NHWC (fp16 or fp32) HBM buffers allocated once per input
shape; the ~60 launches of one forward are replayed as a HIP graph.
"""
from __future__ import annotations

import functools
import math
import os
import re
from typing import List

import torch
import torch.nn as nn

from ..engine import HipModule, Plan
from ..hip_ops import (ActView, FlowtrackHipError, FusedConv, FusedLateralDeconv, PreactConv1x1, Program, record_scale_shift_act, bottleneck_exit_fusable, new_act, new_rowpacked_act,
                       record_bottleneck_exit, record_maxpool, record_pack_input, fold_scale_shift, record_upsample_ac, record_hourglass_down, record_hourglass_up)
from ..params import ActMarker, BatchNormParams, ConvParams, ConvTransposeParams
from ..resnet import BLOCKS, Bottleneck, record_block

resnet_dict = BLOCKS      # depth -> blocks per stage (resnet.py)


class _Stages(dict):
    """plan.stages: the activation view behind each stage.  A stage whose last block was recorded in the exit form
    (DeconvResnet.fuse_stage_exit) may never write its full map: it has no entry, and asking for it says why."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.absent = {}

    def __missing__(self, key):
        if key in self.absent:
            raise FlowtrackHipError(f"plan.stages[{key!r}]: {self.absent[key]}")
        raise KeyError(key)


class PoseResnet(HipModule):
    """What the pose models share: the ResNet trunk and its recording, the plan cache, forward / replay, key points and the flip
    test inside the plan, the exact-arg-max mode.  A model adds its head through three hooks: _make_head (parameters, under the
    reference's names), _init_head (the reference's init_net) and _record_head (the launches from the stage maps to the NCHW fp32
    heat maps)."""
    #: True: the head reads the full maps of layer1..layer3 as well as layer4's, so every stage seam is recorded as today's
    #: launches whatever fuse_stage_exit says (the exit form writes only the even pixels of a stage's last block), and
    #: split_lanes stays off
    full_stage_maps: bool = False
    #: the exact-arg-max mode (exact_in_plan, exact_submit*, forward_keypoint_rows_exact): its error bound was measured for this head
    supports_exact: bool = True
    #: fold each block-0 projection shortcut into its conv3 launch (FusedShortcutConv); FT_FUSE_SHORTCUT=0 keeps them apart
    fuse_shortcut: bool = os.environ.get("FT_FUSE_SHORTCUT", "1") != "0"
    #: identity-shortcut blocks of the 256-wide stage as one launch (ft_bottleneck_fwd); FT_FUSE_BOTTLENECK=0 keeps 3 convs
    fuse_bottleneck: bool = os.environ.get("FT_FUSE_BOTTLENECK", "1") != "0"
    #: a stage's last identity block together with the next stage's conv1 as one launch that writes t1 and only the even pixels of
    #: the block's output (ft_bottleneck_exit_fwd; layer1.2 + layer2.0.conv1): recorded as an alternative to today's launches, the
    #: first-call benchmark keeps one.  FT_FUSE_STAGE_EXIT=0 / False records today's launches only, 2 / "force" the exit form only (dev, tests)
    fuse_stage_exit = {"0": False, "2": "force"}.get(os.environ.get("FT_FUSE_STAGE_EXIT", "1"), True)
    #: the stem's max-pool inside the stem conv launch (ft_conv_desc.pool); FT_FUSE_STEM_POOL=0 keeps the two launches
    fuse_stem_pool: bool = os.environ.get("FT_FUSE_STEM_POOL", "1") != "0"
    #: the fused stem reads the NCHW fp32 input itself (ft_conv_desc.x_nchw_f32): no pack launch, no packed copy, bit-identical
    #: results; FT_FUSE_STEM_PACK=0 keeps ft_pack_nchw_to_nhwc in front of it.  Batch 64 x 256x192, same box: pack 18.7 us + stem 38.5
    #: us -> stem 46.2 us, 59.52 / 59.31 -> 59.71 / 59.61 k crops/s (the first version, predicated global loads instead of
    #: out-of-range buffer loads, ran the stem at 66 us: every load in its own divergent region behind a full wait)
    fuse_stem_pack: bool = os.environ.get("FT_FUSE_STEM_PACK", "1") != "0"
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
    #: dev: layer1 + layer2 as two half-batch lanes (parallel graph branches); FT_SPLIT_LANES=1
    split_lanes4: bool = os.environ.get("FT_SPLIT_LANES4", "0") == "1"       # dev: layer4 as two half-batch lanes
    split_lanes: int = int(os.environ.get("FT_SPLIT_LANES", "0") or 0)     # 1: lanes start together; 2: the second lane starts with its half of the stem
    #: run the 1x1 heatmap conv as the fused tail of the last deconv (fp16 mode); FT_FUSE_HEATMAP=0 keeps it a launch
    fuse_heatmap: bool = os.environ.get("FT_FUSE_HEATMAP", "1") != "0"
    #: forward_keypoint_rows_exact(): a crop is re-run in the fp32 parity arithmetic when ft_heatmap_argmax_screen flags it:
    #: E = exact_argmax_rel_bound x (range of the crop's fp16 heat maps) is taken as the bound of the fp16 mode's heat-map error,
    #: and a crop is flagged when two values of a map are closer than 2 E (an error of at most E per element cannot reorder
    #: values further apart), when a map's maximum is within E of 0 (the `score > 0` coordinate mask of max_preds could flip), or
    #: when anything is non-finite.  The bound is RELATIVE because the error follows the maps' range (the tests bound it as a
    #: fraction of the range); 1.6e-3 = 2 x the largest measured ratio (4.07e-3 on a range of 5.0 = 0.81e-3)
    exact_argmax_rel_bound: float = 1.6e-3

    def __init__(self, layers: List[int], num_classes: int):
        super().__init__()
        self.layers_cfg = list(layers)
        self.num_classes = num_classes
        self.inplanes = 64
        # trunk (resnet.py:19-27)
        self.conv1 = ConvParams(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = BatchNormParams(64)
        self.relu = ActMarker("relu")
        self.maxpool = ActMarker("maxpool3x3s2")
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self._make_head(num_classes)

    def _make_layer(self, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        mods = [Bottleneck(self.inplanes, planes, stride)]
        self.inplanes = planes * 4
        mods += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*mods)

    # -- initialisation / loading (resnet.py:38-49, pose_deconv.py:48-63) ---------------------
    def init_weights(self, pretrained: str = "") -> None:
        if os.path.isfile(pretrained):
            print("=> loading pretrained model {}".format(pretrained))
            self.load_state_dict(torch.load(pretrained, map_location="cpu"), strict=False)
            return
        for m in self.modules():
            if isinstance(m, ConvParams):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, BatchNormParams):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._invalidate()

    def init_net(self, pretrained: str = "") -> None:
        self.init_weights(pretrained)
        self._init_head()
        self._invalidate()

    # -- the head: what a model adds to the trunk -----------------------------------------------
    def _make_head(self, num_classes: int) -> None:
        raise NotImplementedError

    def _init_head(self) -> None:
        raise NotImplementedError

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        """Record the head's launches behind the trunk (`cur` = layer4's map, `stages` the views behind every stage) and return
        the NCHW fp32 heat maps they write."""
        raise NotImplementedError

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

    def _check_exact_supported(self, what: str) -> None:
        if not self.supports_exact:
            raise FlowtrackHipError(f"{what}: the exact-arg-max mode is not available for {type(self).__name__} (its screen's error bound "
                                    "was measured for the deconv head only)")

    def _check_exact_allowed(self, what: str) -> None:
        """Entry check of the exact-arg-max mode: the model has the mode, and no flip test is set."""
        self._check_exact_supported(what)
        self._no_flip(what)

    def _no_flip(self, what: str) -> None:
        if self.flip_pairs is not None:
            raise FlowtrackHipError(f"{what}: flip_pairs is set, and the exact-arg-max mode does not combine with the flip test")

    def _check_input_size(self, H: int, W: int) -> None:
        if H % 32 or W % 32:
            raise FlowtrackHipError(f"input {H}x{W}: height and width must be multiples of 32")

    def _build_plan(self, B: int, H: int, W: int, device, dtype, perm=None) -> Plan:
        """The plan of one input shape: the staged input (and its mirrored half in a flip plan), the network's own launches
        (_record_net: what a model family overrides), then the flip merge / the key points / the exact-arg-max screen."""
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
        if perm is not None:
            # last launch: average the two halves (mirror + left/right swap of the second) and, with keypoints_in_plan, the key points
            # of the merged maps — in place of the separate ft_heatmap_keypoint_rows launch
            K, hh, hw = self.num_classes, heatmaps.shape[2], heatmaps.shape[3]
            merged = torch.empty((B0, K, hh, hw), dtype=torch.float32, device=device)
            plan = Plan(prog, x_static=x_static[:B0], heatmaps=merged)
            plan.stages, plan.heatmaps_raw, plan.x_full = stages, heatmaps, x_static
            plan.flip_perm = torch.tensor(perm, dtype=torch.int32, device=device)
            plan.kp_idx = plan.kp_rows = None
            keep = [merged, heatmaps, plan.flip_perm]
            if self.keypoints_in_plan is not None:
                plan.kp_idx = torch.empty((B0, K), dtype=torch.int32, device=device)
                plan.kp_rows = torch.empty((B0, K, 3), dtype=torch.float32, device=device)
                plan.kp_score, plan.kp_coords = plan.kp_rows[:, :, 2:], plan.kp_rows[:, :, :2]
                keep += [plan.kp_idx, plan.kp_rows]
            prog.add("ft_heatmap_flip_merge", heatmaps.data_ptr(), heatmaps[B0:].data_ptr(), plan.flip_perm.data_ptr(), B0, K, hh, hw,
                     int(bool(self.keypoints_in_plan)), merged.data_ptr(), plan.kp_idx.data_ptr() if plan.kp_idx is not None else None,
                     plan.kp_rows.data_ptr() if plan.kp_rows is not None else None, keep=tuple(keep))
            return plan
        plan = Plan(prog, x_static=x_static, heatmaps=heatmaps)
        plan.stages = stages
        if self.keypoints_in_plan is not None:
            # max_preds (+ the 0.25 px nudge of final_preds) as the last launch of the plan: no extra stream work per call
            K, hh, hw = self.num_classes, heatmaps.shape[2], heatmaps.shape[3]
            # written as (x, y, score) rows — what the tracking glue and the multi-GPU gather consume; scores / coords are views
            plan.kp_idx = torch.empty((B, K), dtype=torch.int32, device=device)
            plan.kp_rows = torch.empty((B, K, 3), dtype=torch.float32, device=device)
            plan.kp_score, plan.kp_coords = plan.kp_rows[:, :, 2:], plan.kp_rows[:, :, :2]
            prog.add("ft_heatmap_keypoint_rows", heatmaps.data_ptr(), B, K, hh, hw, int(bool(self.keypoints_in_plan)),
                     plan.kp_idx.data_ptr(), plan.kp_rows.data_ptr(), keep=(plan.kp_idx, plan.kp_rows))
            if self.exact_in_plan and dtype == torch.float16 and B <= 1024:
                # the exact-arg-max mode's device side INSIDE the plan's graph (round 5): screen -> flag compaction + gather of the
                # flagged crops' inputs -> header {count, indices} to pinned memory.  As graph nodes they cost their kernel time
                # (~10 us); as five eager launches behind the replay they cost ~70 us of gaps per step.  exact_rel_bound is frozen
                # into the plan (DeconvResnet.exact_submit_plan / exact_finish_plan).
                import ctypes
                ex = {"flags": torch.empty(B, dtype=torch.int32, device=device), "stats": torch.empty((B, 4), dtype=torch.float32, device=device),
                      "stage": torch.empty((B, 3, H, W), dtype=torch.float32, device=device),
                      "header": torch.zeros(1 + B, dtype=torch.int32, device=device), "header_host": torch.zeros(1 + B, dtype=torch.int32).pin_memory(),
                      "rel_bound": float(self.exact_argmax_rel_bound), "event": None, "busy": False}
                prog.add("ft_heatmap_argmax_screen", heatmaps.data_ptr(), B, K, hh, hw, ctypes.c_float(ex["rel_bound"]), ex["flags"].data_ptr(),
                         ex["stats"].data_ptr(), keep=(ex["flags"], ex["stats"]))
                prog.add("ft_gather_flagged_rows", ex["flags"].data_ptr(), B, x_static.data_ptr(), ctypes.c_longlong(3 * H * W * 4), ex["stage"].data_ptr(),
                         ex["header"].data_ptr(), keep=(ex["stage"], ex["header"]))
                prog.add("ft_memcpy_async", ex["header_host"].data_ptr(), ex["header"].data_ptr(), ctypes.c_size_t((1 + B) * 4), keep=(ex["header_host"],))
                plan.exact = ex
        return plan

    def _record_net(self, prog, x_static, dtype, device):
        """Record everything between "the input is staged in x_static [B,3,H,W] fp32" and "the heat maps exist": returns (stages,
        the NCHW fp32 heat maps the plan's tail reads).  Here: the ResNet trunk and, through _record_head, the model's head."""
        B, _, H, W = x_static.shape
        mk = dict(dtype=dtype, device=device)
        # 7x7/s2/p3 stem: one kernel row = one K-run.  fp16: conv1 + bn1 + relu + maxpool (resnet.py:19-23) are ONE launch
        # (ft_conv_desc.pool; its patch starts one stem column further left: 5 physical pad columns instead of 3) and the
        # [B, H/2, W/2, 64] stem map never exists
        pool_in_stem = self.fuse_stem_pool and dtype == torch.float16
        planar_in = pool_in_stem and self.fuse_stem_pack      # the stem gathers its patches from x_static: a_in is geometry only
        a_in = new_rowpacked_act(B, H, W, 3, 5 if pool_in_stem else 3, dtype, "meta" if planar_in else device)
        if not planar_in:
            record_pack_input(prog, x_static, a_in)
        xs = (lambda lo, hi: x_static[lo:hi]) if planar_in else (lambda lo, hi: None)

        stem = self.fused("conv1" + ("+maxpool" if pool_in_stem else ""), self.conv1.weight, stride=2, pad=3, bn=self.bn1.as_dict(),
                          act="relu", **mk)
        cur = new_act(B, H // 4, W // 4, 64, dtype, device)
        split = self.split_lanes if (dtype == torch.float16 and B % 2 == 0 and B >= 32 and pool_in_stem and not self.full_stage_maps) else 0
        if split == 2:
            stem.record(prog, a_in.batch_slice(0, B // 2), cur.batch_slice(0, B // 2), pool=True, x_nchw=xs(0, B // 2))     # (the other half: on the second lane)
        elif pool_in_stem:
            stem.record(prog, a_in, cur, pool=True, x_nchw=xs(0, B))
        else:
            a1 = new_act(B, H // 2, W // 2, 64, dtype, device)
            stem.record(prog, a_in, a1)
            record_maxpool(prog, a1, cur)

        # FT_SPLIT_LANES=1 (dev, measured in profiles/README.md): layer1 + layer2 as TWO half-batch lanes (parallel graph branches).
        # Their fused blocks are phase-locked across the chip — every workgroup reads its input, then multiplies, then writes, at
        # the same time, so HBM idles while the matrix pipe runs and vice versa; two lanes half a block apart overlap them.
        stages = _Stages({"stem": cur})         # activation views behind each stage (diagnostics: tests/error_budget.py)
        trunk = (self.layer1, self.layer2, self.layer3, self.layer4)
        seam = None                    # output view of this stage's entry block when the previous stage's exit form recorded it
        for li, layer in enumerate(trunk, start=1):
            if li > 1 and seam is None:
                stages[f"layer{li - 1}"] = cur
            elif li > 1:
                stages.absent[f"layer{li - 1}"] = ("this plan records the stage's last block in the exit form, which writes only the even pixels of "
                                                   "its output (the full map exists only if the first-call benchmark kept today's launches): for the "
                                                   "map, build the model with fuse_stage_exit = False (FT_FUSE_STAGE_EXIT=0)")
            if split and li == 1:
                # (split == 2: the side lane starts with its half of the stem: half a block of useful delay, the lanes' memory and
                # matrix phases interleave)
                side_stem = functools.partial(stem.record, prog, a_in.batch_slice(B // 2, B), cur.batch_slice(B // 2, B), pool=True,
                                              x_nchw=xs(B // 2, B)) if split == 2 else None
                cur = self._record_lanes(prog, [(f"layer{lj}.{bi}", blk) for lj, lay in ((1, self.layer1), (2, self.layer2)) for bi, blk in enumerate(lay)],
                                         cur, side_stem)
                continue
            if split and li == 2:
                continue
            if self.split_lanes4 and li == 4 and dtype == torch.float16 and B % 2 == 0 and B >= 32:
                # FT_SPLIT_LANES4=1 (dev): layer4 as two half-batch lanes.  Its nine launches are small (15-30 us each, of which ~6 us
                # are the launch's ramp with the chip mostly idle: cd_phases.py shows 10-us workgroup lifetimes in 16-us kernels); two
                # lanes fill each other's ramps, and halving the pixels halves the workgroups, not the weight bytes per workgroup.
                # MEASURED (two interleaved bench runs): 56.37 / 55.82 -> 53.75 / 53.79 k crops/s: off.
                cur = self._record_lanes(prog, [(f"layer4.{bi}", blk) for bi, blk in enumerate(layer)], cur)
                continue
            for bi, blk in enumerate(layer):
                if bi == 0 and seam is not None:
                    cur, seam = seam, None
                    continue
                name = f"layer{li}.{bi}"
                out = new_act(B, cur.H // blk.stride, cur.W // blk.stride, blk.conv1.cout * 4, dtype, device)
                if bi == len(layer) - 1 and bi > 0 and li < 4 and not split and not self.full_stage_maps:
                    seam = self._record_stage_exit(prog, name, blk, f"layer{li + 1}.0", trunk[li][0], cur, out, dtype, device)
                    if seam is not None:
                        continue
                cur = self._record_trunk_block(prog, name, blk, cur, out)

        stages["layer4"] = cur
        heatmaps = self._record_head(prog, stages, cur, dtype, device)
        return stages, heatmaps

    def _record_lanes(self, prog, blocks, cur: ActView, side_first=None) -> ActView:
        """The chain `blocks` = [(name, blk), ...] from view `cur` as two half-batch lanes (parallel graph branches): the first half
        on the main lane, the second on the side lane, behind `side_first()` where given.  Returns the chain's full-batch output."""
        B, chain = cur.N, []
        hh, ww = cur.H, cur.W
        for name, blk in blocks:
            hh, ww = hh // blk.stride, ww // blk.stride
            chain.append((name, blk, new_act(B, hh, ww, blk.conv1.cout * 4, cur.t.dtype, cur.t.device)))

        def lane(lo, hi):
            c = cur.batch_slice(lo, hi)
            for name, blk, out_full in chain:
                c = self._record_trunk_block(prog, name, blk, c, out_full.batch_slice(lo, hi))
        prog.fork()
        lane(0, B // 2)
        with prog.side():
            if side_first is not None:
                side_first()
            lane(B // 2, B)
        prog.join()
        return chain[-1][2]

    def _record_trunk_block(self, prog, name: str, blk, cur: ActView, out: ActView) -> ActView:
        """One trunk block (stride on its 3x3) in every form this model's switches offer: resnet.record_block."""
        forms = (("fused", "entry", "head", "head2") if self.fuse_bottleneck else ()) + (("shortcut",) if self.fuse_shortcut else ()) + \
            (("cluster",) if self.cluster_kernels else ()) + (("strips",) if self.strip_kernels else ())
        return record_block(self, prog, name, blk, cur, out, stride=blk.stride, stride_on="conv2", forms=forms)

    def _record_stage_exit(self, prog, name: str, blk, nname: str, nblk, cur, out, dtype, device):
        """The seam between two stages: `blk` = the stage's last identity block (from `cur` into `out`), `nblk` = the stride-2 entry
        block of the next stage.  Nothing but nblk.conv1 and nblk's stride-2 shortcut reads `out`, so where ft_bottleneck_exit_fwd
        covers the pair (fp16, 256 -> 64 -> 64 -> 256 then 256 -> 128: layer1 -> layer2) two forms of BOTH blocks are recorded and
        the first-call benchmark keeps one:
          "fused"  blk + nblk.conv1 as one launch that writes t1 and the even pixels of blk's output as a compact half-size map,
                   then nblk.conv2 and the K-concatenated conv3 + shortcut, which reads the compact map at stride 1;
          "convs"  the launches resnet.record_block gives the two blocks (nblk.conv1 a launch of its own).
        Returns nblk's output view, or None when the exit form does not apply (nothing recorded then)."""
        if not (self.fuse_stage_exit and self.fuse_bottleneck and self.fuse_shortcut) or dtype != torch.float16:
            return None
        if len(blk.downsample) or blk.stride != 1 or nblk.stride != 2 or not len(nblk.downsample) or cur.H % 2 or cur.W % 2:
            return None
        B, mk = cur.N, dict(dtype=dtype, device=device)
        nplanes = nblk.conv1.cout
        c1 = self.fused(name + ".conv1", blk.conv1.weight, bn=blk.bn1.as_dict(), act="relu", **mk)
        c2 = self.fused(name + ".conv2", blk.conv2.weight, stride=1, pad=1, bn=blk.bn2.as_dict(), act="relu", **mk)
        c3 = self.fused(name + ".conv3", blk.conv3.weight, bn=blk.bn3.as_dict(), act="relu", **mk)
        n1 = self.fused(nname + ".conv1", nblk.conv1.weight, bn=nblk.bn1.as_dict(), act="relu", **mk)
        n2 = self.fused(nname + ".conv2", nblk.conv2.weight, stride=2, pad=1, bn=nblk.bn2.as_dict(), act="relu", **mk)
        t1 = new_act(B, cur.H, cur.W, nplanes, dtype, device)
        y_even = new_act(B, cur.H // 2, cur.W // 2, cur.C, dtype, device)
        if not bottleneck_exit_fusable(c1, c2, c3, n1, cur, y_even, t1, "even"):
            return None
        t2 = new_act(B, cur.H // 2, cur.W // 2, nplanes, dtype, device)
        nout = new_act(B, cur.H // 2, cur.W // 2, nplanes * 4, dtype, device)
        # the same GEMM as the block recorder's, its shortcut operand read at stride 1 from the compact map
        sc = self.fused_shortcut(nname + ".conv3+downsample", nblk, 1, key_suffix="@even", **mk)

        def exit_form():
            record_bottleneck_exit(prog, c1, c2, c3, n1, cur, y_even, t1, f"{name}.fused+{nname}.conv1", "even")
            n2.record(prog, t1, t2)
            sc.record(prog, t2, y_even, nout)

        def block_form():
            self._record_trunk_block(prog, name, blk, cur, out)
            self._record_trunk_block(prog, nname, nblk, out, nout)
        if self.fuse_stage_exit == "force":
            exit_form()
            return nout
        # a choice of the "bottleneck" family, with that family's option names: "fused" = the block fused with the conv behind it
        # (the exit form), "convs" = that conv stays a launch of its own (today's launches of the two blocks)
        prog.begin_choice(f"bottleneck|exit,{B},{cur.H},{cur.W},{cur.C},{nplanes},{cur.cstride}")
        for form_name, form in (("fused", exit_form), ("convs", block_form)):
            prog.option(form_name)
            form()
        prog.end_choice()
        return nout

    #: offer the cluster form of the 256-plane identity blocks (ft_bottleneck_cluster_fwd) to the first-call benchmark
    #: (FT_CLUSTER_KERNELS=1).  OFF by default: measured in situ at R50 batch 64 it takes 50-52 us per block against the strip
    #: form's 48 (each of its two in-launch hand-offs costs 4-5 us: profiles/README.md, round 5), and its workgroups wait for
    #: each other inside the launch (bounded spins: nothing deadlocks, but a timed-out hand-off gives a wrong block).
    cluster_kernels: bool = os.environ.get("FT_CLUSTER_KERNELS", "0") == "1"
    strip_kernels: bool = os.environ.get("FT_STRIP_KERNELS", "0") in ("1", "2")      # the 64-plane block's register-stationary form as an option

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


    # ---- the exact-arg-max mode without a host read inside the step (round 5) -------------------------------------------------
    # forward_keypoint_rows_exact() reads the B flags on the host between the fp16 plan and the re-run: with nothing flagged that
    # read (a stream synchronisation per step) cost 10 % of the step.  Here the step ends on the device: fp16 plan -> screen ->
    # ft_gather_flagged_rows (flag compaction + copy of the flagged crops' INPUTS into a staging slot, all on the device) -> an
    # asynchronous copy of the small header {count, indices} to pinned memory -> event.  exact_finish(), called one step later
    # (or whenever the caller needs the rows), waits for that event — long past — and only if the count is non-zero runs the fp32
    # plan on the staged crops and patches their rows.  The caller's x may be overwritten as soon as exact_submit() returns.
    def _exact_slots(self, B: int, H: int, W: int, device):
        key = (B, H, W, str(device))
        st = self.__dict__.setdefault("_exact_state", {})
        ent = st.get(key)
        if ent is None:
            import ctypes
            from .. import _lib
            lib = _lib.load()
            slots = []
            for _ in range(2):
                ev = ctypes.c_void_p()
                if lib.ft_event_create(ctypes.byref(ev)) != 0:
                    raise FlowtrackHipError("ft_event_create failed")
                slots.append({"stage": torch.empty((B, 3, H, W), dtype=torch.float32, device=device),
                              "flags": torch.empty(B, dtype=torch.int32, device=device), "stats": torch.empty((B, 4), dtype=torch.float32, device=device),
                              "header": torch.zeros(1 + B, dtype=torch.int32, device=device),
                              "header_host": torch.zeros(1 + B, dtype=torch.int32).pin_memory(), "event": ev, "busy": False})
            ent = st[key] = {"slots": slots, "next": 0}
        return ent

    def release_exact_state(self) -> None:
        """Destroy the events and drop the pinned headers / staging buffers of the asynchronous exact-arg-max paths (exact_submit
        slots and the per-plan state of exact_submit_plan).  Called when the plans are invalidated (weights, dtype or device changed)
        and by close(); a step that is still in flight is abandoned (its handle must not be finished afterwards)."""
        from .. import _lib
        lib = _lib.load() if (self.__dict__.get("_exact_state") or any(getattr(pl, "exact", None) for pl in self.__dict__.get("_plans", {}).values())) else None
        for ent in self.__dict__.get("_exact_state", {}).values():
            for sl in ent["slots"]:
                if sl.get("event") is not None:
                    lib.ft_event_destroy(sl["event"])
                    sl["event"] = None
        self.__dict__["_exact_state"] = {}
        for pl in self.__dict__.get("_plans", {}).values():
            ex = getattr(pl, "exact", None)
            if ex and ex.get("event") is not None:
                lib.ft_event_destroy(ex["event"])
                ex["event"], ex["busy"] = None, False

    def _invalidate(self):
        self.release_exact_state()
        super()._invalidate()

    def close(self) -> None:
        """Release what the module holds outside torch's allocator (events of the exact-arg-max paths) and its captured plans."""
        self._invalidate()

    @torch.no_grad()
    def exact_submit(self, x: torch.Tensor) -> "_ExactHandle":
        """First half of the exact-arg-max step (see above): everything is queued on the current stream, nothing is waited for."""
        if self.keypoints_in_plan is None:
            raise FlowtrackHipError("set model.keypoints_in_plan = True / False (adjust_coords) before exact_submit()")
        self._check_exact_allowed("exact_submit")
        import ctypes
        from .. import _lib
        from ..hip_ops import check, current_stream_handle
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
        import ctypes
        from .. import _lib
        from ..hip_ops import check, current_stream_handle
        lib = _lib.load()
        if ex["event"] is None:
            ev = ctypes.c_void_p()
            check(lib.ft_event_create(ctypes.byref(ev)), "ft_event_create")
            ex["event"] = ev
        self.replay(plan)
        check(lib.ft_event_record(ex["event"], current_stream_handle(plan.x_static.device)), "ft_event_record")
        ex["busy"] = True
        return plan

    @torch.no_grad()
    def exact_finish_plan(self, plan: Plan):
        """(plan.kp_rows with the flagged crops' rows replaced by the fp32 parity mode's, number of crops re-run)."""
        from .. import _lib
        from ..hip_ops import check
        ex = plan.exact
        if not ex["busy"]:
            raise FlowtrackHipError("exact_finish_plan: nothing submitted")
        try:
            check(_lib.load().ft_event_synchronize(ex["event"]), "ft_event_synchronize")
            n = int(ex["header_host"][0])
            if n:
                B, _, H, W = plan.x_static.shape
                self._rerun_flagged(ex["header_host"], ex["stage"], plan.kp_rows, n, B, H, W)
        finally:
            ex["busy"] = False
        return plan.kp_rows, n

    def _rerun_flagged(self, hdr, stage, rows, n, B, H, W):
        """The n flagged crops (inputs staged in `stage`, indices in hdr[1:]) through the fp32 plan; their rows patched into `rows`."""
        dev = rows.device
        idx = hdr[1:1 + n].to(torch.int64).to(dev)
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
                xb[:take].copy_(stage[lo:lo + take])
                if take < bucket:
                    xb[take:].zero_()
                r32 = self.forward_keypoint_rows(xb)
                rows.index_copy_(0, idx[lo:lo + take], r32[:take])
                lo += take
        finally:
            self.compute_dtype, self.exact_in_plan = want, ex_flag

    @torch.no_grad()
    def exact_finish(self, h: "_ExactHandle"):
        """Second half: (rows [B,K,3] with the parity mode's arg-max, number of crops re-run in fp32)."""
        if h.done:
            raise FlowtrackHipError("exact_finish: handle already finished")
        from .. import _lib
        from ..hip_ops import check
        lib = _lib.load()
        dev = h.rows.device
        ent = self._exact_slots(h.B, h.H, h.W, dev)
        sl = ent["slots"][h.slot]
        check(lib.ft_event_synchronize(sl["event"]), "ft_event_synchronize")
        hdr = sl["header_host"]
        n = int(hdr[0])
        h.done = True
        try:
            if n:
                self._rerun_flagged(hdr, sl["stage"], h.rows, n, h.B, h.H, h.W)
        finally:
            sl["busy"] = False       # an exception inside the fp32 re-run must not pin the slot
        return h.rows, n

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
        import ctypes
        from .. import _lib
        from ..hip_ops import check, current_stream_handle
        B = x.shape[0]
        self.compute_dtype = torch.float16
        try:
            rows = self.forward_keypoint_rows(x).clone()
            plan = self._last_plan
            hm = plan.heatmaps
            flags = torch.empty(B, dtype=torch.int32, device=x.device)
            stats = torch.empty((B, 4), dtype=torch.float32, device=x.device)
            check(_lib.load().ft_heatmap_argmax_screen(hm.data_ptr(), B, hm.shape[1], hm.shape[2], hm.shape[3],
                                                       ctypes.c_float(self.exact_argmax_rel_bound), flags.data_ptr(), stats.data_ptr(),
                                                       current_stream_handle(x.device)), "ft_heatmap_argmax_screen")
            self._last_screen_stats = stats
            todo = torch.nonzero(flags.cpu()).flatten()
            n = int(todo.numel())
            if n:
                self.compute_dtype = torch.float32
                todo_dev = todo.to(x.device)
                lo = 0
                while lo < n:
                    m = min(n - lo, B)
                    bucket = next(b for b in (8, 16, 32, 64, 128, 256, 1 << 30) if b >= m or b >= B)
                    bucket = min(bucket, max(B, 8))
                    xb = self.static_input(bucket, x.shape[2], x.shape[3])
                    sel = todo_dev[lo:lo + min(m, bucket)]
                    xb[:len(sel)].copy_(x.index_select(0, sel))
                    if len(sel) < bucket:
                        xb[len(sel):].zero_()
                    r32 = self.forward_keypoint_rows(xb)
                    rows.index_copy_(0, sel, r32[:len(sel)])
                    lo += len(sel)
        finally:
            self.compute_dtype = want
        return rows, n


class _ExactHandle:
    __slots__ = ("rows", "slot", "B", "H", "W", "done")


class DeconvResnet(PoseResnet):
    """ResNet trunk + 3 x ConvTranspose(4,2,1) + 1x1 heatmap conv (pose_deconv.py:12-63)."""

    def _make_head(self, num_classes: int) -> None:
        # head (pose_deconv.py:16-30)
        self.deconv_bias = False
        feats = 256
        self.deconv = nn.Sequential(
            ConvTransposeParams(2048, feats, bias=False), BatchNormParams(feats), ActMarker("relu"),
            ConvTransposeParams(feats, feats, bias=False), BatchNormParams(feats), ActMarker("relu"),
            ConvTransposeParams(feats, feats, bias=False), BatchNormParams(feats), ActMarker("relu"))
        self.heatmap = ConvParams(feats, num_classes, 1, bias=True)

    def _init_head(self) -> None:
        for m in self.deconv:
            if isinstance(m, ConvTransposeParams):
                nn.init.normal_(m.weight, std=0.001)
            elif isinstance(m, BatchNormParams):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.heatmap.weight, std=0.001)
        nn.init.constant_(self.heatmap.bias, 0)

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        # head: 3 x (ConvTranspose 4/2/1 + bn + relu), then the 1x1 heatmap conv (pose_deconv.py:43-45) — fused behind
        # the last deconv as its tail in fp16 mode: the [B, 64, 48, 256] map, the largest tensor of the head, never
        # reaches HBM
        B, mk = cur.N, dict(dtype=dtype, device=device)
        fuse_tail = self.fuse_heatmap and dtype == torch.float16 and self.num_classes <= 32 and self.deconv[6].cout in (64, 128, 256)
        heatmaps = None
        for i in (0, 3, 6):
            tail = dict(tail_weight=self.heatmap.weight, tail_bias=self.heatmap.bias) if (i == 6 and fuse_tail) else {}
            dc = self.fused(f"deconv.{i}" + ("+heatmap" if tail else ""), self.deconv[i].weight, transposed=True, stride=2, pad=1,
                            bias=self.deconv[i].bias, bn=self.deconv[i + 1].as_dict(), act="relu", **tail, **mk)
            if tail:
                heatmaps = torch.empty((B, self.num_classes, cur.H * 2, cur.W * 2), dtype=torch.float32, device=device)
                dc.record(prog, cur, heatmaps)
            else:
                nxt = new_act(B, cur.H * 2, cur.W * 2, dc.cout, dtype, device)
                dc.record(prog, cur, nxt)
                cur = nxt
                stages[f"deconv.{i}"] = cur
        if heatmaps is None:
            hm = self.fused("heatmap", self.heatmap.weight, bias=self.heatmap.bias, act=None, **mk)
            heatmaps = torch.empty((B, self.num_classes, cur.H, cur.W), dtype=torch.float32, device=device)
            hm.record(prog, cur, heatmaps)
        return heatmaps


def _bn_relu_conv(cin: int, cout: int, kernel_size: int, padding: int = 0, bias: bool = True) -> nn.Sequential:
    """_make_conv of pose_fpn.py:41-46: BatchNorm, ReLU, conv — pre-activation order, so index 0 is the BN and 2 the conv."""
    return nn.Sequential(BatchNormParams(cin), ActMarker("relu"), ConvParams(cin, cout, kernel_size, padding=padding, bias=bias))


class FpnResnet(PoseResnet):
    """ResNet trunk + FPN top-down path + 1x1 heatmap conv (pose_fpn.py:48-104).  With c2..c5 the maps behind layer1..layer4:

        p5 = latlayer1(c5)
        p4 = toplayer1(up(p5) + latlayer2(c4)),  p3 = toplayer2(up(p4) + latlayer3(c3)),  p2 = toplayer3(up(p3) + latlayer4(c2))
        heatmaps = heatmap(p2)                      toplayer_j, heatmap = BatchNorm -> ReLU -> conv;  up = bilinear, align_corners=True

    Each top-down step is three launches.  With (s, b) the fold of toplayer_j's BatchNorm,
    relu(bn(up(p) + lat(c))) = relu(s * lat(c) + b + s * up(p)): ft_upsample_bilinear_ac_fwd writes u = s * up(p), the lateral 1x1 conv
    takes s, b as its scale / shift and u as its residual input, and toplayer_j's 3x3 conv reads the activated map (its zero padding
    pads that map, as in the reference).  Nothing else reads the un-normalised sum.  The last 3x3 conv carries heatmap.0's BatchNorm
    and ReLU in its epilogue, since only the heatmap conv reads p2."""
    full_stage_maps = True
    supports_exact = False

    def _make_head(self, num_classes: int) -> None:
        feats = 256
        for i, cin in enumerate((2048, 1024, 512, 256), start=1):       # lateral layers (pose_fpn.py:54-58)
            setattr(self, f"latlayer{i}", ConvParams(cin, feats, 1, bias=False))
        for j in (1, 2, 3):                                             # top-down layers (pose_fpn.py:60-63)
            setattr(self, f"toplayer{j}", _bn_relu_conv(feats, feats, 3, padding=1, bias=False))
        self.heatmap = _bn_relu_conv(feats, num_classes, 1)

    def _init_head(self) -> None:
        # pose_fpn.py:92-104
        for name, m in self.named_modules():
            if "lat" in name or "top" in name:
                if isinstance(m, ConvParams):
                    nn.init.normal_(m.weight, std=0.001)
                elif isinstance(m, BatchNormParams):
                    nn.init.constant_(m.weight, 1)
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.heatmap[2].weight, std=0.001)
        nn.init.constant_(self.heatmap[2].bias, 0)

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        B, mk = cur.N, dict(dtype=dtype, device=device)
        feats = self.latlayer1.cout
        p = new_act(B, cur.H, cur.W, feats, dtype, device)
        self._record_p5(prog, cur, p, dtype, device)
        stages["p5"] = p
        for j, stage in ((1, "layer3"), (2, "layer2"), (3, "layer1")):
            lat, top, c = getattr(self, f"latlayer{j + 1}"), getattr(self, f"toplayer{j}"), stages[stage]
            bn = top[0].as_dict()
            key = (f"toplayer{j}.0.scale", dtype, str(device))
            scale = self._layers.get(key)
            if scale is None:
                scale = self._layers[key] = fold_scale_shift(feats, feats, None, bn, device)[0]
            u = new_act(B, c.H, c.W, feats, dtype, device)
            record_upsample_ac(prog, p, u, scale)
            a = new_act(B, c.H, c.W, feats, dtype, device)
            self.fused(f"latlayer{j + 1}+toplayer{j}.0", lat.weight, bn=bn, act="relu", **mk).record(prog, c, a, residual=u)
            last = j == 3
            conv = self.fused(f"toplayer{j}.2" + ("+heatmap.0" if last else ""), top[2].weight, pad=1,
                              bn=self.heatmap[0].as_dict() if last else None, act="relu" if last else None, **mk)
            p = new_act(B, c.H, c.W, feats, dtype, device)
            conv.record(prog, a, p)
            stages[f"p{5 - j}"] = p
        heatmaps = torch.empty((B, self.num_classes, p.H, p.W), dtype=torch.float32, device=device)
        self.fused("heatmap.2", self.heatmap[2].weight, bias=self.heatmap[2].bias, act=None, **mk).record(prog, p, heatmaps)
        return heatmaps


    def _record_p5(self, prog, cur: ActView, p: ActView, dtype, device) -> None:
        """p5 = latlayer1(c5) from the trunk's last map `cur` (here c5 itself)."""
        self.fused("latlayer1", self.latlayer1.weight, act=None, dtype=dtype, device=device).record(prog, cur, p)


#: depth -> (num_init_features, growth_rate, block_config) (densenet.py:150-153)
densenet_dict = {121: (64, 32, [6, 12, 24, 16]), 169: (64, 32, [6, 12, 32, 32]), 201: (64, 32, [6, 12, 48, 32]), 161: (96, 48, [6, 12, 36, 24])}


class DenseLayer(nn.Module):
    """Parameter layout of _DenseLayer (densenet.py:19-30): norm1 -> relu1 -> conv1 (1x1 to bn_size * growth) -> norm2 -> relu2 -> conv2
    (3x3 to growth); its output is concatenated behind its input."""

    def __init__(self, cin: int, growth: int, bn_size: int):
        super().__init__()
        self.norm1, self.relu1 = BatchNormParams(cin), ActMarker("relu")
        self.conv1 = ConvParams(cin, bn_size * growth, 1, bias=False)
        self.norm2, self.relu2 = BatchNormParams(bn_size * growth), ActMarker("relu")
        self.conv2 = ConvParams(bn_size * growth, growth, 3, padding=1, bias=False)


class DenseBlock(nn.Module):
    """_DenseBlock (densenet.py:39-44): denselayer1 .. denselayerN, layer i on cin + (i - 1) growth channels."""

    def __init__(self, num_layers: int, cin: int, growth: int, bn_size: int):
        super().__init__()
        for i in range(num_layers):
            self.add_module(f"denselayer{i + 1}", DenseLayer(cin + i * growth, growth, bn_size))

    def layers(self):
        return list(self.children())


class Transition(nn.Module):
    """_Transition (densenet.py:47-54): norm -> relu -> conv (1x1, halves the channels) -> AvgPool2d(2, 2)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.norm, self.relu = BatchNormParams(cin), ActMarker("relu")
        self.conv = ConvParams(cin, cout, 1, bias=False)
        self.pool = ActMarker("avgpool2x2s2")


class FpnDensenet(FpnResnet):
    """DenseNet-BC trunk + the FPN head of FpnResnet (pose_fpn.py:106-151, densenet.py:57-108).  Of PoseResnet it keeps everything
    behind the network itself (the plan cache, forward / replay, the flip plan, the key points inside the plan), of FpnResnet the
    head; the parameters and the trunk's launch list (_record_net) are its own, and none of the ResNet trunk's switches applies.

    A dense block is ONE NHWC buffer [B, H, W, inplanes + L * growth]: every layer reads the channel window [0, cin) and writes its
    `growth` new channels into the window behind it, so the reference's torch.cat never runs.  A dense layer is two launches:
        t = relu(norm2(conv1(relu(norm1(block[:cin])))))      ft_preact_conv1x1_fwd: norm1 + ReLU on the GEMM's input operand (norm1
                                                               belongs to the layer that reads the concat: no producer can fold it)
        block[cin : cin + growth] = conv2(t)                   the 3x3 conv of today's path
    The first is recorded in two forms, the first-call benchmark keeps one per shape (`dense_layer_form` pins one):
      "preact"        the one launch above;
      "affine+igemm"  ft_scale_shift_act_nhwc_fwd writes relu(norm1(block[:cin])), ft_conv2d_fwd reads it.
    A transition is one ft_preact_conv1x1_fwd launch with pool = 1 (the 2x2 average commutes with the 1x1 conv, so it runs on the
    GEMM's input and the GEMM has a quarter of the pixels) into channels [0, inplanes / 2) of the next block's buffer; p5 =
    latlayer1(relu(norm5(block4))) is one more, so c5 is never written.  latlayer2..4 read the raw block buffers c4, c3, c2."""
    #: None: both forms of a dense layer's first launch are recorded and the first-call benchmark keeps one per shape; "preact" /
    #: "affine+igemm" records that form only (dev, tests; FT_DENSE_LAYER in the environment)
    dense_layer_form = os.environ.get("FT_DENSE_LAYER") or None
    LAYER_FORMS = ("preact", "affine+igemm")
    bn_size = 4

    def __init__(self, num_init_features: int, growth_rate: int, block_config, num_classes: int):
        HipModule.__init__(self)        # (not PoseResnet's: that one builds the ResNet trunk)
        self.num_classes, self.growth_rate, self.block_config = num_classes, growth_rate, list(block_config)
        self.conv0 = ConvParams(3, num_init_features, 7, stride=2, padding=3, bias=False)
        self.norm0 = BatchNormParams(num_init_features)
        self.relu0 = ActMarker("relu")
        self.pool0 = ActMarker("maxpool3x3s2")
        self.inplanes, self.planes = num_init_features, []
        for i, n in enumerate(self.block_config):
            setattr(self, f"denseblock{i + 1}", DenseBlock(n, self.inplanes, growth_rate, self.bn_size))
            self.inplanes += n * growth_rate
            self.planes.append(self.inplanes)
            if i != len(self.block_config) - 1:
                setattr(self, f"transition{i + 1}", Transition(self.inplanes, self.inplanes // 2))
                self.inplanes //= 2
        self.norm5 = BatchNormParams(self.inplanes)
        feats = 256
        for i in range(4):                                              # lateral layers (pose_fpn.py:113-116): latlayer1 reads c5
            setattr(self, f"latlayer{i + 1}", ConvParams(self.planes[3 - i], feats, 1, bias=False))
        for j in (1, 2, 3):
            setattr(self, f"toplayer{j}", _bn_relu_conv(feats, feats, 3, padding=1, bias=False))
        self.heatmap = _bn_relu_conv(feats, num_classes, 1)

    # -- initialisation / loading (densenet.py:122-148) -------------------------------------------
    _OLD_KEY = re.compile(r"^(.*denselayer\d+\.(?:norm|relu|conv))\.((?:[12])\.(?:weight|bias|running_mean|running_var))$")

    @classmethod
    def rewrite_checkpoint_keys(cls, state_dict: dict) -> dict:
        """torchvision's DenseNet checkpoints under this model's names: `features.` stripped, `norm.1` -> `norm1` and likewise
        (densenet.py:126-139)."""
        out = {}
        for key, v in state_dict.items():
            new_key = re.sub(r"^features\.", "", key)
            m = cls._OLD_KEY.match(new_key)
            if m:
                new_key = m.group(1) + m.group(2)
            out[new_key] = v
        return out

    def init_weights(self, pretrained: str = "") -> None:
        if os.path.isfile(pretrained):
            print("=> loading pretrained model {}".format(pretrained))
            self.load_state_dict(self.rewrite_checkpoint_keys(torch.load(pretrained, map_location="cpu")), strict=False)
            return
        for m in self.modules():
            if isinstance(m, ConvParams):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, BatchNormParams):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._invalidate()

    def _check_input_size(self, H: int, W: int) -> None:
        if H % 32 or W % 32 or H < 64 or W < 64:
            raise FlowtrackHipError(f"input {H}x{W}: height and width must be multiples of 32 and at least 64")

    # -- the launch list ----------------------------------------------------------------------------
    def _preact(self, label: str, weight, pre_bn, post_bn, act, dtype, device) -> PreactConv1x1:
        key = (label, dtype, str(device))
        layer = self._layers.get(key)
        if layer is None:
            layer = self._layers[key] = PreactConv1x1(weight, pre_bn.as_dict(), post_bn=post_bn.as_dict() if post_bn is not None else None,
                                                      act=act, dtype=dtype, device=device, label=label)
        return layer

    def _record_p5(self, prog, cur: ActView, p: ActView, dtype, device) -> None:
        """p5 = latlayer1(relu(norm5(block4))): norm5 + ReLU on the input operand, the activated map c5 is never written."""
        self._preact("norm5+latlayer1", self.latlayer1.weight, self.norm5, None, None, dtype, device).record(prog, cur, p)

    def _record_net(self, prog, x_static, dtype, device):
        form = self.dense_layer_form
        if form is not None and form not in self.LAYER_FORMS:
            raise FlowtrackHipError(f"dense_layer_form {form!r}: None or one of {self.LAYER_FORMS}")
        B, _, H, W = x_static.shape
        mk = dict(dtype=dtype, device=device)
        growth, c0 = self.growth_rate, self.conv0.cout
        h, w = H // 4, W // 4
        buf = new_act(B, h, w, self.planes[0], dtype, device)
        stem_out = ActView(buf.t, c0, 0)
        # conv0 + norm0 + relu0 + pool0 into channels [0, c0) of block 1's buffer; fp16: one launch, as PoseResnet's stem
        pool_in_stem = self.fuse_stem_pool and dtype == torch.float16
        planar_in = pool_in_stem and self.fuse_stem_pack
        a_in = new_rowpacked_act(B, H, W, 3, 5 if pool_in_stem else 3, dtype, "meta" if planar_in else device)
        if not planar_in:
            record_pack_input(prog, x_static, a_in)
        stem = self.fused("conv0" + ("+pool0" if pool_in_stem else ""), self.conv0.weight, stride=2, pad=3, bn=self.norm0.as_dict(), act="relu", **mk)
        if pool_in_stem:
            stem.record(prog, a_in, stem_out, pool=True, x_nchw=x_static if planar_in else None)
        else:
            a1 = new_act(B, H // 2, W // 2, c0, dtype, device)
            stem.record(prog, a_in, a1)
            pooled = new_act(B, h, w, c0, dtype, device)
            record_maxpool(prog, a1, pooled)
            # (the max-pool kernel writes dense buffers: its map goes into the block's window as x * 1 + 0, exactly)
            key = ("pool0.copy", dtype, str(device))
            ident = self._layers.get(key)
            if ident is None:
                ident = self._layers[key] = (torch.ones(c0, dtype=torch.float32, device=device), torch.zeros(c0, dtype=torch.float32, device=device))
            record_scale_shift_act(prog, pooled, stem_out, ident[0], ident[1], None)
        stages = _Stages({"stem": stem_out})
        cin = c0
        for bi, nlayers in enumerate(self.block_config, start=1):
            block = getattr(self, f"denseblock{bi}")
            t = new_act(B, h, w, self.bn_size * growth, dtype, device)             # conv1's output: read by the next launch only
            scratch = new_act(B, h, w, self.planes[bi - 1], dtype, device) if form != "preact" else None
            for li, layer in enumerate(block.layers(), start=1):
                name = f"denseblock{bi}.denselayer{li}"
                pc = self._preact(name + ".norm1+conv1+norm2", layer.conv1.weight, layer.norm1, layer.norm2, "relu", dtype, device)
                c2 = self.fused(name + ".conv2", layer.conv2.weight, pad=1, act=None, **mk)
                xin = ActView(buf.t, cin, 0)
                forms = {"preact": lambda pc=pc, xin=xin: pc.record(prog, xin, t),
                         "affine+igemm": lambda pc=pc, xin=xin: pc.record_unfused(prog, xin, t, ActView(scratch.t, xin.C, 0))}
                if form is not None:
                    forms[form]()
                else:
                    prog.begin_choice(f"dense_layer|{B},{h},{w},{cin},{t.C},{buf.cstride},{dtype}")
                    for fname in self.LAYER_FORMS:
                        prog.option(fname)
                        forms[fname]()
                    prog.end_choice()
                c2.record(prog, t, ActView(buf.t, growth, cin))
                cin += growth
            stages[f"layer{bi}"] = buf
            if bi != len(self.block_config):
                tr = getattr(self, f"transition{bi}")
                h, w = h // 2, w // 2
                nxt = new_act(B, h, w, self.planes[bi], dtype, device)
                self._preact(f"transition{bi}", tr.conv.weight, tr.norm, None, None, dtype, device).record(prog, buf, ActView(nxt.t, cin // 2, 0), pool=True)
                buf, cin = nxt, cin // 2
        heatmaps = self._record_head(prog, stages, buf, dtype, device)
        return stages, heatmaps


def _bn_relu_deconv(cin: int, cout: int) -> nn.Sequential:
    """_make_deconv of pose_net.py:9-14: BatchNorm (over the INPUT channels), ReLU, ConvTranspose2d(4,2,1) without bias."""
    return nn.Sequential(BatchNormParams(cin), ActMarker("relu"), ConvTransposeParams(cin, cout, bias=False))


class LateralDeconvResnet(PoseResnet):
    """ResNet trunk + three `BatchNorm -> ReLU -> ConvTranspose2d(4,2,1)` steps, each summed with a 1x1 lateral conv of the trunk
    map at its output's scale, + `BatchNorm -> ReLU -> 1x1` heat maps (pose_net.py:30-91).  With c2..c5 the maps behind layer1..layer4:

        p4 = deconv1(c5) + latlayer2(c4),  p3 = deconv2(p4) + latlayer3(c3),  p2 = deconv3(p3) + latlayer4(c2),  heatmaps = heatmap(p2)

    Nothing reads a sum p_j but the BatchNorm + ReLU in front of the next layer, so with (s, b) the fold of that BatchNorm
    (deconv2.0, deconv3.0, heatmap.0) the plan holds only the activated maps:

        a5 = relu(bn_deconv1.0(c5))                       ft_scale_shift_act_nhwc_fwd (c5 is layer4's activated output: no epilogue to fold into)
        a4 = relu(s (deconv1(a5) + lat2(c4)) + b)         one step, likewise a3 and a2
        heatmaps = heatmap.2(a2) + bias                   1x1 conv to NCHW fp32

    A step is recorded in two forms, the first-call benchmark keeps one (`lateral_step_form` forces one):
      "kconcat"         ONE launch: the lateral conv as one more K-run of each parity phase of the transposed conv (FusedLateralDeconv);
      "lateral+deconv"  two launches: the lateral conv writes l = s lat(c) + b, the transposed conv takes scale s, no shift, l as its
                        residual input and the ReLU — on whatever kernel today's dispatch gives a transposed conv with a residual.
    The heat-map conv stays a launch of its own: the fused tail, x2 and a residual all use the same pointer argument."""
    full_stage_maps = True
    supports_exact = False
    #: None: both forms of a top-down step are recorded and the first-call benchmark keeps one; "kconcat" / "lateral+deconv" records
    #: that form only (dev, tests; FT_LATERAL_STEP in the environment)
    lateral_step_form = os.environ.get("FT_LATERAL_STEP") or None
    STEP_FORMS = ("kconcat", "lateral+deconv")

    def _make_head(self, num_classes: int) -> None:
        feats = 256
        for i, cin in ((2, 1024), (3, 512), (4, 256)):                   # lateral layers (pose_net.py:36-40): there is no latlayer1
            setattr(self, f"latlayer{i}", ConvParams(cin, feats, 1, bias=False))
        for j, cin in ((1, 2048), (2, feats), (3, feats)):               # top-down layers (pose_net.py:42-45)
            setattr(self, f"deconv{j}", _bn_relu_deconv(cin, feats))
        self.heatmap = _bn_relu_conv(feats, num_classes, 1)

    def _init_head(self) -> None:
        # pose_net.py:69-91
        for name, m in self.named_modules():
            if "lat" in name:
                if isinstance(m, ConvParams):
                    nn.init.normal_(m.weight, std=0.001)
            elif "deconv" in name:
                if isinstance(m, ConvTransposeParams):
                    nn.init.normal_(m.weight, std=0.001)
                elif isinstance(m, BatchNormParams):
                    nn.init.constant_(m.weight, 1)
                    nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.heatmap[0].weight, 1)
        nn.init.constant_(self.heatmap[0].bias, 0)
        nn.init.normal_(self.heatmap[2].weight, std=0.001)
        nn.init.constant_(self.heatmap[2].bias, 0)

    def _record_head(self, prog, stages, cur, dtype, device) -> torch.Tensor:
        form = self.lateral_step_form
        if form is not None and form not in self.STEP_FORMS:
            raise FlowtrackHipError(f"lateral_step_form {form!r}: None or one of {self.STEP_FORMS}")
        B, mk = cur.N, dict(dtype=dtype, device=device)
        feats = self.latlayer2.cout
        key = ("deconv1.0.scale_shift", dtype, str(device))
        ss = self._layers.get(key)
        if ss is None:
            ss = self._layers[key] = fold_scale_shift(cur.C, cur.C, None, self.deconv1[0].as_dict(), device)
        a = new_act(B, cur.H, cur.W, cur.C, dtype, device)
        record_scale_shift_act(prog, cur, a, ss[0], ss[1], "relu")
        stages["a5"] = a
        steps = ((1, 2, "layer3", self.deconv2[0]), (2, 3, "layer2", self.deconv3[0]), (3, 4, "layer1", self.heatmap[0]))
        for j, i, stage, bn_mod in steps:
            dc, lat, c = getattr(self, f"deconv{j}")[2], getattr(self, f"latlayer{i}"), stages[stage]
            bn = bn_mod.as_dict()
            name = f"deconv{j}.2+latlayer{i}"
            out = new_act(B, c.H, c.W, feats, dtype, device)
            key = (name, dtype, str(device))
            kc = self._layers.get(key)
            if kc is None:
                kc = self._layers[key] = FusedLateralDeconv(dc.weight, lat.weight, bn, act="relu", label=name, **mk)
            # the two-launch form's layers: l = s lat(c) + b (no activation), then relu(s deconv(a) + l)
            lat_conv = self.fused(f"latlayer{i}.bn", lat.weight, bn=bn, act=None, **mk)
            key = (f"deconv{j}.2.scaled", dtype, str(device))
            dc_conv = self._layers.get(key)
            if dc_conv is None:
                no_shift = dict(bn, bias=torch.zeros_like(bn["bias"]), running_mean=torch.zeros_like(bn["running_mean"]))
                dc_conv = self._layers[key] = FusedConv(dc.weight, transposed=True, stride=2, pad=1, bn=no_shift, act="relu",
                                                        label=f"deconv{j}.2+residual", **mk)
            lbuf = new_act(B, c.H, c.W, feats, dtype, device)

            def kconcat_form(kc=kc, a=a, c=c, out=out):
                kc.record(prog, a, c, out)

            def two_form(lat_conv=lat_conv, dc_conv=dc_conv, a=a, c=c, out=out, lbuf=lbuf):
                lat_conv.record(prog, c, lbuf)
                dc_conv.record(prog, a, out, residual=lbuf)
            forms = {"kconcat": kconcat_form, "lateral+deconv": two_form}
            if form is not None:
                forms[form]()
            else:
                prog.begin_choice(f"lateral_step|{B},{a.H},{a.W},{a.C},{c.C},{feats},{a.cstride},{c.cstride},{dtype}")
                for fname in self.STEP_FORMS:
                    prog.option(fname)
                    forms[fname]()
                prog.end_choice()
            a = out
            stages[f"a{5 - j}"] = a
        heatmaps = torch.empty((B, self.num_classes, a.H, a.W), dtype=torch.float32, device=device)
        self.fused("heatmap.2", self.heatmap[2].weight, bias=self.heatmap[2].bias, act=None, **mk).record(prog, a, heatmaps)
        return heatmaps


class HgBottleneck(nn.Module):
    """Parameter layout of the hourglass's pre-activation block (hourglass.py:10-45): out = branch(relu(bn(x))) + shortcut(x) with
    branch = 1x1 -> bn -> relu -> 3x3 -> bn -> relu -> 1x1 at half the output's planes; `shortcut` is a 1x1 conv where the channel
    count changes, and the 'no_preact' form (res1, behind the stem's own ReLU) has no `preact`."""

    def __init__(self, inplanes: int, outplanes: int, preact: bool = True, bias: bool = True):
        super().__init__()
        planes = outplanes // 2
        self.shortcut = ConvParams(inplanes, outplanes, 1, bias=bias) if inplanes != outplanes else None
        if preact:
            self.preact = nn.Sequential(BatchNormParams(inplanes), ActMarker("relu"))
        self.branch = nn.Sequential(ConvParams(inplanes, planes, 1, bias=bias), BatchNormParams(planes), ActMarker("relu"),
                                    ConvParams(planes, planes, 3, padding=1, bias=bias), BatchNormParams(planes), ActMarker("relu"),
                                    ConvParams(planes, outplanes, 1, bias=bias))


def _hg_residual(inplanes: int, outplanes: int, num_blocks: int, preact: bool = True) -> nn.Sequential:
    """_make_residual (hourglass.py:56-63,175-182): num_blocks blocks, the first one carries the change of width."""
    return nn.Sequential(HgBottleneck(inplanes, outplanes, preact), *[HgBottleneck(outplanes, outplanes) for _ in range(1, num_blocks)])


class Hourglass(nn.Module):
    """Parameter layout of one hourglass (hourglass.py:47-74): hg[d] = the three chains of level d + 1 (up, low1, low3), and a
    fourth (low2) at the lowest level d = 0."""

    def __init__(self, num_blocks: int, planes: int, depth: int):
        super().__init__()
        self.depth = depth
        self.maxpool = ActMarker("maxpool2x2s2")
        self.hg = nn.ModuleList(nn.ModuleList(_hg_residual(planes, planes, num_blocks) for _ in range(4 if d == 0 else 3))
                                for d in range(depth))


class HourglassNet(PoseResnet):
    """The stacked hourglass (hourglass.py:127-231; Newell et al., ECCV 2016) on the HIP path.  Of PoseResnet it keeps everything
    behind the network itself — the plan cache, forward / replay, the flip plan, the key points inside the plan — and replaces the
    parameters and the launch list (_record_net); none of the ResNet trunk's switches applies.

        x = res3(res2(maxpool(res1(pre(input)))))                                            [B, H/4, W/4, 256]
        per stack i:  y = proj[i](res[i](hg[i](x)));  heatmap_i = heatmap[i](y);  x = x + proj_[i](y) + heatmap_[i](heatmap_i)
        hg level n:   up1 = hg[n-1][0](x);  low1 = hg[n-1][1](maxpool(x));  low2 = level n-1 (low1), or hg[0][3](low1) at n = 1
                      out = up1 + upsample_ac(hg[n-1][2](low2), size of up1)

    Every block is pre-activation: conv1 reads relu(bn(x)), the residual add reads x.  A block is three conv launches — 1x1 + bn +
    relu, 3x3 + bn + relu, 1x1 + bias + residual (no activation) — and its activated input comes from where its raw input is made:
      ft_hourglass_down_fwd  at the top of every level reads the level's input once and writes a_full (for hg[n-1][0]), the pooled
                             map and its activated copy (for hg[n-1][1]); behind res1 it writes the pooled pair only;
      ft_hourglass_up_fwd    at the end of every level writes the sum (in place of up1) and its activated copy for the next block
                             (hg[n][2] of the level above, res[i] at the top);
      ft_scale_shift_act_nhwc_fwd  only where the input is a conv3 output: inside chains of more than one block, hg[0][3], the
                             lowest hg[0][2], res3.
    fuse_seams = False records the same arithmetic unfused (pool alone, sum alone, stand-alone activations): the fused outputs
    are bit-identical to it (tests/test_hourglass_gpu.py).  The join between stacks is two convs chained through the residual
    input; stack i's heat map is written twice by the same layer, NCHW fp32 for the caller and NHWC as heatmap_[i]'s input."""
    supports_exact = False
    #: write the activated copies at the level seams (ft_hourglass_down_fwd / ft_hourglass_up_fwd) instead of stand-alone launches
    fuse_seams: bool = True
    depth, num_feats = 4, 256

    def __init__(self, num_classes: int, num_stacks: int, num_blocks: int):
        HipModule.__init__(self)        # (not PoseResnet's: that one builds the ResNet trunk)
        self.num_classes, self.num_stacks, self.num_blocks = num_classes, num_stacks, num_blocks
        feats = self.num_feats
        self.pre = nn.Sequential(ConvParams(3, 64, 7, stride=2, padding=3, bias=True), BatchNormParams(64), ActMarker("relu"))
        self.res1 = _hg_residual(64, 256, 1, preact=False)
        self.res2 = _hg_residual(256, 256, 1)
        self.res3 = _hg_residual(256, feats, 1)
        self.maxpool = ActMarker("maxpool2x2s2")
        self.hg = nn.ModuleList(Hourglass(num_blocks, feats, self.depth) for _ in range(num_stacks))
        self.res = nn.ModuleList(_hg_residual(feats, feats, num_blocks) for _ in range(num_stacks))
        self.proj = nn.ModuleList(nn.Sequential(ConvParams(feats, feats, 1), BatchNormParams(feats), ActMarker("relu")) for _ in range(num_stacks))
        self.heatmap = nn.ModuleList(ConvParams(feats, num_classes, 1) for _ in range(num_stacks))
        self.proj_ = nn.ModuleList(ConvParams(feats, feats, 1) for _ in range(num_stacks - 1))
        self.heatmap_ = nn.ModuleList(ConvParams(num_classes, feats, 1) for _ in range(num_stacks - 1))
        self.init_weights()

    # -- initialisation (hourglass.py:166-173): the constructor's, there is no init_net in the reference ------------------------
    def init_weights(self, pretrained: str = "") -> None:
        if pretrained and os.path.isfile(pretrained):
            print("=> loading pretrained model {}".format(pretrained))
            self.load_state_dict(torch.load(pretrained, map_location="cpu"), strict=False)
            return
        for m in self.modules():
            if isinstance(m, ConvParams):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, BatchNormParams):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._invalidate()

    def _init_head(self) -> None:
        pass

    def _check_input_size(self, H: int, W: int) -> None:
        low = 1 << self.depth
        if H % 4 or W % 4 or H // 4 < low or W // 4 < low:
            raise FlowtrackHipError(f"input {H}x{W}: height and width must be multiples of 4 and at least {4 * low} (the map of the "
                                    f"hourglass's lowest level, 1/{4 * low} of the input rounded down, must not be empty)")

    @torch.no_grad()
    def forward(self, x: torch.Tensor, copy_output: bool = True) -> List[torch.Tensor]:
        """x: [B,3,H,W] on the model's GPU -> the reference's list of num_stacks heat-map tensors [B,K,H/4,W/4] fp32, one per
        stack (hourglass.py:203-225); the last one is what plans, the flip test and the key points are built on."""
        self._forward(x, False, None)
        maps = [self._last_plan.stages[f"heatmap.{i}"] for i in range(self.num_stacks)]
        return [t.clone() for t in maps] if copy_output else maps

    # -- the launch list --------------------------------------------------------------------------------------------------------
    def _bn_table(self, name: str, bn, dtype, device):
        """(scale, shift) fp32 [C] of an eval-mode BatchNorm for the element-wise kernels, folded once per (dtype, device)."""
        key = (name + ".scale_shift", dtype, str(device))
        tab = self._layers.get(key)
        if tab is None:
            tab = self._layers[key] = fold_scale_shift(bn.num_features, bn.num_features, None, bn.as_dict(), device)
        return tab

    def _record_net(self, prog, x_static, dtype, device):
        B, _, H, W = x_static.shape
        mk = dict(dtype=dtype, device=device)
        stages = _Stages()
        scratch = {}

        def tmp(tag, h, w, c):          # t1 / t2 of a block: read by the next launch only, so one buffer per size serves every block
            key = (tag, h, w, c)
            if key not in scratch:
                scratch[key] = new_act(B, h, w, c, dtype, device)
            return scratch[key]

        def act_of(name, blk, raw):     # stand-alone relu(bn(raw)) for block `name`
            a = new_act(B, raw.H, raw.W, raw.C, dtype, device)
            record_scale_shift_act(prog, raw, a, *self._bn_table(name + ".preact.0", blk.preact[0], dtype, device), "relu")
            return a

        def block(name, blk, raw, a):
            br = blk.branch
            c1 = self.fused(name + ".branch.0", br[0].weight, bias=br[0].bias, bn=br[1].as_dict(), act="relu", **mk)
            c2 = self.fused(name + ".branch.3", br[3].weight, pad=1, bias=br[3].bias, bn=br[4].as_dict(), act="relu", **mk)
            c3 = self.fused(name + ".branch.6", br[6].weight, bias=br[6].bias, act=None, **mk)
            t1, t2 = tmp("t1", raw.H, raw.W, c1.cout), tmp("t2", raw.H, raw.W, c2.cout)
            c1.record(prog, a, t1)
            c2.record(prog, t1, t2)
            res = raw
            if blk.shortcut is not None:        # res1's 64 -> 256 projection: a conv of its own that feeds the residual input
                res = new_act(B, raw.H, raw.W, c3.cout, dtype, device)
                self.fused(name + ".shortcut", blk.shortcut.weight, bias=blk.shortcut.bias, act=None, **mk).record(prog, raw, res)
            out = new_act(B, raw.H, raw.W, c3.cout, dtype, device)
            c3.record(prog, t2, out, residual=res)
            return out

        def chain(name, seq, raw, a):   # a = the first block's activated input where a seam wrote it, else None
            for k, blk in enumerate(seq):
                bname = f"{name}.{k}"
                if a is None:
                    a = act_of(bname, blk, raw)
                raw, a = block(bname, blk, raw, a), None
            return raw

        def down(x, tab_pool, tab_full):
            pool = new_act(B, x.H // 2, x.W // 2, x.C, dtype, device)
            a_pool = new_act(B, x.H // 2, x.W // 2, x.C, dtype, device)
            a_full = new_act(B, x.H, x.W, x.C, dtype, device) if tab_full is not None else None
            if self.fuse_seams:
                record_hourglass_down(prog, x, pool, a_pool, tab_pool, a_full, tab_full)
            else:
                record_hourglass_down(prog, x, pool)
                if a_full is not None:
                    record_scale_shift_act(prog, x, a_full, *tab_full, "relu")
                record_scale_shift_act(prog, pool, a_pool, *tab_pool, "relu")
            return pool, a_pool, a_full

        def level(i, n, x, tab_next):
            """Level n of hourglass i on the raw map x -> (out, relu(bn_next(out)))."""
            mods, name = self.hg[i].hg[n - 1], f"hg.{i}.hg.{n - 1}"
            pool, a_pool, a_full = down(x, self._bn_table(name + ".1.0.preact.0", mods[1][0].preact[0], dtype, device),
                                        self._bn_table(name + ".0.0.preact.0", mods[0][0].preact[0], dtype, device))
            up1 = chain(name + ".0", mods[0], x, a_full)
            low1 = chain(name + ".1", mods[1], pool, a_pool)
            if n > 1:
                low2, a_low2 = level(i, n - 1, low1, self._bn_table(name + ".2.0.preact.0", mods[2][0].preact[0], dtype, device))
            else:
                low2, a_low2 = chain(name + ".3", mods[3], low1, None), None
            low3 = chain(name + ".2", mods[2], low2, a_low2)
            a_out = new_act(B, up1.H, up1.W, up1.C, dtype, device)
            if self.fuse_seams:
                record_hourglass_up(prog, up1, low3, up1, a_out, tab_next)      # (the sum takes up1's place: nothing else reads up1)
            else:
                record_hourglass_up(prog, up1, low3, up1)
                record_scale_shift_act(prog, up1, a_out, *tab_next, "relu")
            return up1, a_out

        # pre = 7x7/s2/p3 conv + bias + bn + relu on the row-packed input (one kernel row = one K-run), res1, the 2x2 pool, res2, res3
        a_in = new_rowpacked_act(B, H, W, 3, 3, dtype, device)
        record_pack_input(prog, x_static, a_in)
        p = new_act(B, H // 2, W // 2, 64, dtype, device)
        self.fused("pre", self.pre[0].weight, stride=2, pad=3, bias=self.pre[0].bias, bn=self.pre[1].as_dict(), act="relu", **mk).record(prog, a_in, p)
        stages["pre"] = p
        r1 = chain("res1", self.res1, p, p)             # 'no_preact': the block reads the stem's activated map as it is
        stages["res1"] = r1
        pool, a_pool, _ = down(r1, self._bn_table("res2.0.preact.0", self.res2[0].preact[0], dtype, device), None)
        x = chain("res3", self.res3, chain("res2", self.res2, pool, a_pool), None)
        stages["res3"] = x
        K = self.num_classes
        heatmaps = None
        for i in range(self.num_stacks):
            y, a_y = level(i, self.depth, x, self._bn_table(f"res.{i}.0.preact.0", self.res[i][0].preact[0], dtype, device))
            stages[f"hg.{i}"] = y
            y = chain(f"res.{i}", self.res[i], y, a_y)
            y2 = new_act(B, y.H, y.W, self.num_feats, dtype, device)
            self.fused(f"proj.{i}", self.proj[i][0].weight, bias=self.proj[i][0].bias, bn=self.proj[i][1].as_dict(), act="relu", **mk).record(prog, y, y2)
            hm = self.fused(f"heatmap.{i}", self.heatmap[i].weight, bias=self.heatmap[i].bias, act=None, **mk)
            heatmaps = torch.empty((B, K, y.H, y.W), dtype=torch.float32, device=device)
            hm.record(prog, y2, heatmaps)
            stages[f"heatmap.{i}"] = heatmaps
            if i < self.num_stacks - 1:
                # x + proj_(y) + heatmap_(heatmap): the heat map once more as an NHWC map of the compute type (its pad channels
                # [K, 32 k) stay zero: the conv reads them against zero weights), then two convs chained through the residual input
                hm_nhwc = new_act(B, y.H, y.W, K, dtype, device, cstride=(K + 31) // 32 * 32)
                hm.record(prog, y2, hm_nhwc)
                t = new_act(B, y.H, y.W, self.num_feats, dtype, device)
                self.fused(f"proj_.{i}", self.proj_[i].weight, bias=self.proj_[i].bias, act=None, **mk).record(prog, y2, t, residual=x)
                xn = new_act(B, y.H, y.W, self.num_feats, dtype, device)
                self.fused(f"heatmap_.{i}", self.heatmap_[i].weight, bias=self.heatmap_[i].bias, act=None, **mk).record(prog, hm_nhwc, xn, residual=t)
                x = xn
                stages[f"stack.{i}"] = x
        return stages, heatmaps


def deconv(backbone: str, num_classes: int, pretrained: bool) -> DeconvResnet:
    """Factory with the reference's signature (pose_deconv.py:166-179): backbone 'resnet50' |
    'resnet101' | 'resnet152'; pretrained=True loads data/pretrained/<backbone>.pth if present."""
    if not backbone.startswith("resnet"):
        raise FlowtrackHipError(f"backbone '{backbone}': only the ResNet-50/101/152 + deconv head is on the HIP path")
    depth = int(backbone[len("resnet"):])
    if depth not in resnet_dict:
        raise FlowtrackHipError(f"resnet{depth}: the deconv head needs a Bottleneck trunk (50/101/152)")
    model = DeconvResnet(resnet_dict[depth], num_classes=num_classes)
    path = os.path.join("data", "pretrained", "{}.pth".format(backbone)) if pretrained else ""
    model.init_net(path)
    return model


def fpn(backbone: str, num_classes: int, pretrained: bool) -> FpnResnet:
    """Factory with the reference's signature (pose_fpn.py:171-184) for backbone 'resnet50' | 'resnet101' | 'resnet152';
    pretrained=True loads data/pretrained/<backbone>.pth if present.  The reference's DenseNet trunks: fpn_densenet."""
    depth = backbone[len("resnet"):] if backbone.startswith("resnet") else ""
    if not depth.isdigit() or int(depth) not in resnet_dict:
        raise FlowtrackHipError(f"backbone '{backbone}': the FPN head is on the HIP path for resnet50 / resnet101 / resnet152 only" +
                                ("; DenseNet trunks: models.fpn_densenet" if backbone.startswith("densenet") else ""))
    model = FpnResnet(resnet_dict[int(depth)], num_classes=num_classes)
    path = os.path.join("data", "pretrained", "{}.pth".format(backbone)) if pretrained else ""
    model.init_net(path)
    return model


#: DenseNet trunks of fpn_densenet.  densenet161 (growth 48) is not among them: its channel windows (144, 240, ...) are no multiples
#: of 32, the K-step of the channel-aligned 3x3 conv kernel that every other trunk's windows run on, and that path has not been
#: validated on such windows
FPN_DENSENETS = ("densenet121", "densenet169", "densenet201")


def fpn_densenet(backbone: str, num_classes: int, pretrained: bool) -> FpnDensenet:
    """The reference's models.fpn on its DenseNet trunks (pose_fpn.py:106-184) for backbone 'densenet121' | 'densenet169' |
    'densenet201'; pretrained=True loads data/pretrained/<backbone>.pth if present (a torchvision checkpoint: its keys are rewritten
    as densenet.py:126-139 rewrites them)."""
    if backbone == "densenet161":
        raise FlowtrackHipError("backbone 'densenet161': growth rate 48 gives channel windows (144, 240, ...) that are no multiples of 32; the 3x3 "
                                f"conv kernel of the HIP path has not been validated on them.  Accepted: {' / '.join(FPN_DENSENETS)}")
    if backbone not in FPN_DENSENETS:
        raise FlowtrackHipError(f"backbone '{backbone}': fpn_densenet takes {' / '.join(FPN_DENSENETS)}")
    model = FpnDensenet(*densenet_dict[int(backbone[len("densenet"):])], num_classes=num_classes)
    path = os.path.join("data", "pretrained", "{}.pth".format(backbone)) if pretrained else ""
    model.init_net(path)
    return model


def pose(backbone: str, num_classes: int, pretrained: bool) -> LateralDeconvResnet:
    """Factory with the reference's signature (pose_net.py:163-177) for backbone 'resnet50' | 'resnet101' | 'resnet152';
    pretrained=True loads data/pretrained/<backbone>.pth if present.  The reference's own DenseNet form of this model cannot be
    built (pose_net.py:101 names an undefined `bias`), so there is nothing to follow for it."""
    if backbone.startswith("densenet"):
        raise FlowtrackHipError(f"backbone '{backbone}': the reference itself cannot build this model (PoseDensenet raises NameError: "
                                "name 'bias' is not defined); the lateral-deconv head is on the HIP path for resnet50 / resnet101 / resnet152 only")
    depth = backbone[len("resnet"):] if backbone.startswith("resnet") else ""
    if not depth.isdigit() or int(depth) not in resnet_dict:
        raise FlowtrackHipError(f"backbone '{backbone}': the lateral-deconv head is on the HIP path for resnet50 / resnet101 / resnet152 only")
    model = LateralDeconvResnet(resnet_dict[int(depth)], num_classes=num_classes)
    path = os.path.join("data", "pretrained", "{}.pth".format(backbone)) if pretrained else ""
    model.init_net(path)
    return model


def hg(num_classes: int, num_stacks: int) -> HourglassNet:
    """Factory with the reference's signature (hourglass.py:227-231): num_stacks hourglasses of depth 4 on 256 features with
    8 // num_stacks blocks per chain, every conv with bias; the constructor's init is the reference's (there is no checkpoint path)."""
    if isinstance(num_stacks, bool) or not isinstance(num_stacks, int) or not 1 <= num_stacks <= 8:
        raise FlowtrackHipError(f"num_stacks {num_stacks!r}: an integer from 1 to 8 (the reference builds 8 // num_stacks blocks per chain)")
    return HourglassNet(num_classes, num_stacks, 8 // num_stacks)
