"""The Faster R-CNN person detector of FlowTrack on the HIP path, inference only, on two of the reference's trunks: the
Caffe-strided ResNet-50/101/152 (region head: layer4 on the RoI crops) and VGG16 (region head: the two 4096-wide FCs).

Drop-in surface (reference lib/detection: nets/resnet_v1.py: resnetv1, nets/vgg16.py: vgg16, the inference half of nets/network.py:
Network):
    net = resnetv1(num_layers=50) | vgg16(); net.create_architecture(num_classes, tag='default', anchor_scales, anchor_ratios)
    net.state_dict() / load_state_dict(sd) / load_pretrained_cnn(sd) / .cuda() / .eval()
    net.test_image(image[1,H,W,3] fp32 blob, im_info) -> (cls_score, cls_prob, bbox_pred, rois) as numpy; net._predictions
    net.extract_head(image) -> net_conv [1,1024 | 512,h,w] fp32
    net.compute_dtype = torch.float32 (the parity mode) / torch.float16, as the pose models switch
forward(mode='TRAIN') and everything that needs targets or losses raise FlowtrackHipError.

Two plans (hip_ops.Program launch lists, replayed as HIP graphs) per blob shape and dtype:
    trunk + RPN   pack -> the trunk -> rpn_net -> the two RPN heads as ONE 1x1 GEMM with 6A outputs ->
                  fp32 copies of the score and box channels -> ft_rpn_softmax_fwd
        resnetv1  conv1 -> max-pool -> layer1..layer3
        vgg16     13 x (3x3 conv + bias + ReLU) with ft_maxpool2x2s2_fwd behind convs 2, 4, 7 and 10 (nets/vgg16.py:38: the last
                  max-pool of `features` is not run)
    region head   ft_roi_crop_nhwc_fwd at post_nms_topN rows -> the trunk's tail -> cls_score_net and
                  bbox_pred_net as ONE GEMM with 5 * num_classes fp32 outputs
        resnetv1  crop at 7x7 -> layer4 (N = rows) -> ft_rcnn_mean_pool_fwd
        vgg16     crop at 14x14 + 2x2 max (max_pool = 1, nets/network.py:93) -> classifier.0 + ReLU -> classifier.3 + ReLU (dropout is
                  the identity in eval; nets/vgg16.py:31: there is no classifier.6).  In fp16 each FC is recorded as a choice between
                  ft_conv2d_fwd on the [rows,1,1,K] view ("igemm", first: the faster form at 300 rows) and ft_fc_fwd ("fc");
                  fp32 keeps "igemm"
Between them: detection.proposal.proposal_layer (its one device -> host read: the kept count); rows past that count carry zero
RoIs and are dropped.  Behind them: ft_rcnn_detections_fwd (class softmax, un-normalised deltas, and for im_detect the boxes).
Everything that does not depend on the trunk lives in _FasterRCNN.
detect_enqueue is the same frame step with nothing read from the device (proposal.proposal_layer_device between the plans,
ft_detect_select_fwd behind them): what detection.test.detect_persons_clip enqueues for every frame of a clip.

The blob has any height and width, so every map size follows (n + 2p - k) // s + 1 (the VGG pools: n // 2) and odd maps occur at
every stage.  The ResNet block recorder (resnet.record_block, shared with the pose trunks) takes a fused form only where the
library's query accepts the shape: ft_bottleneck_fwd / ft_bottleneck_stream_fwd for identity blocks (bottleneck_fusable), the
K-concatenated conv3 + shortcut GEMM (FusedShortcutConv.supported); everything else is plain ft_conv2d_fwd launches and
ft_maxpool3x3s2_fwd.  The stem's fused max-pool and the stage-exit form have no query that covers odd maps and are not recorded here.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._lib import FlowtrackHipError, check
from ..engine import HipModule, Plan
from ..hip_ops import (ActView, FusedFC, Program, current_stream_handle, new_act, new_rowpacked_act, record_maxpool, record_maxpool2x2,
                       record_pack_input)
from ..params import ActMarker, BatchNormParams, ConvParams, LinearParams
from ..resnet import BLOCKS, Bottleneck, conv_out, record_block
from . import proposal

__all__ = ["resnetv1", "vgg16", "BLOCKS", "BBOX_NORMALIZE_STDS", "BBOX_NORMALIZE_MEANS"]

BBOX_NORMALIZE_STDS = (0.1, 0.1, 0.2, 0.2)      # model/config.py: TRAIN.BBOX_NORMALIZE_STDS
BBOX_NORMALIZE_MEANS = (0.0, 0.0, 0.0, 0.0)     # TRAIN.BBOX_NORMALIZE_MEANS
FEAT_STRIDE = 16
RPN_CHANNELS = 512                               # model/config.py: RPN_CHANNELS
VGG_CFG_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")     # torchvision's vgg16


class _ResNet(nn.Module):
    """Parameter layout of torchvision's ResNet without avgpool / fc (nets/resnet_v1.py:25-37)."""

    def __init__(self, layers):
        super().__init__()
        self.conv1 = ConvParams(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = BatchNormParams(64)
        self.relu = ActMarker("relu")
        self.maxpool = ActMarker("maxpool3x3s2")
        inplanes = 64
        for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), layers), start=1):
            mods = [Bottleneck(inplanes, planes, 1 if li == 1 else 2)]
            inplanes = planes * 4
            mods += [Bottleneck(inplanes, planes) for _ in range(1, blocks)]
            setattr(self, f"layer{li}", nn.Sequential(*mods))


class _VGG(nn.Module):
    """Parameter layout of torchvision's VGG (config D, no BatchNorm) with fc8 removed (nets/vgg16.py:29-31): convs at features
    0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28 with markers at the ReLU / max-pool positions, Linear layers at classifier 0 and 3
    with markers at the ReLU / dropout positions."""

    def __init__(self):
        super().__init__()
        mods, cin = [], 3
        for v in VGG_CFG_D:
            if v == "M":
                mods.append(ActMarker("maxpool2x2s2"))
            else:
                mods += [ConvParams(cin, v, 3, padding=1), ActMarker("relu")]
                cin = v
        self.features = nn.Sequential(*mods)
        self.classifier = nn.Sequential(LinearParams(512 * 7 * 7, 4096), ActMarker("relu"), ActMarker("dropout"),
                                        LinearParams(4096, 4096), ActMarker("relu"), ActMarker("dropout"))


class _FasterRCNN(HipModule):
    """What the detectors share (nets/network.py: Network, inference half): the five head layers and their init, the RPN steps
    behind net_conv, the class / box GEMM behind fc7, the two plan caches and everything that runs them.  A trunk provides
    _init_head_tail(), load_pretrained_cnn(), _record_trunk(prog, plan, H, W, device, dtype) -> net_conv,
    _record_tail(prog, plan, net_conv, rows, device, dtype) -> fc7 and _plan_switches() (what of its recording switches keys a plan)."""

    #: overrides of cfg.TEST.RPN_PRE_NMS_TOP_N / RPN_POST_NMS_TOP_N / RPN_NMS_THRESH (None: 6000 / 300 / 0.7)
    rpn_pre_nms_topN = None
    rpn_post_nms_topN = None
    rpn_nms_thresh = None

    def __init__(self):
        super().__init__()
        self._feat_stride = [FEAT_STRIDE]
        self._predictions = {}

    # -- construction (nets/network.py:286-317) ------------------------------------------------------------------------------
    def create_architecture(self, num_classes, tag=None, anchor_scales=(8, 16, 32), anchor_ratios=(0.5, 1, 2)):
        self._tag = tag
        self._num_classes = int(num_classes)
        self._anchor_scales, self._anchor_ratios = tuple(anchor_scales), tuple(anchor_ratios)
        self._num_anchors = len(self._anchor_scales) * len(self._anchor_ratios)
        self._init_head_tail()
        self.rpn_net = ConvParams(self._net_conv_channels, RPN_CHANNELS, 3, padding=1)
        self.rpn_cls_score_net = ConvParams(RPN_CHANNELS, self._num_anchors * 2, 1)
        self.rpn_bbox_pred_net = ConvParams(RPN_CHANNELS, self._num_anchors * 4, 1)
        self.cls_score_net = LinearParams(self._fc7_channels, self._num_classes)
        self.bbox_pred_net = LinearParams(self._fc7_channels, self._num_classes * 4)
        self.init_weights()

    def init_weights(self):
        """nets/network.py:393-409: N(0, 0.01) for the head layers, N(0, 0.001) for bbox_pred_net, zero biases."""
        with torch.no_grad():
            for m, std in ((self.rpn_net, 0.01), (self.rpn_cls_score_net, 0.01), (self.rpn_bbox_pred_net, 0.01), (self.cls_score_net, 0.01),
                           (self.bbox_pred_net, 0.001)):
                m.weight.normal_(0, std)
                m.bias.zero_()
        self._invalidate()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """nets/network.py:481-487: exactly this net's keys are read, extra ones (an old checkpoint's resnet.fc.*) are ignored; a
        missing one is a KeyError.  `strict` is accepted for nn.Module's signature and has no effect: the rule above is the reference's
        and is always the strict load of exactly this net's keys."""
        return super().load_state_dict({k: state_dict[k] for k in list(self.state_dict())}, strict=True)

    # -- recording -------------------------------------------------------------------------------------------------------------
    def _record_rpn(self, prog, plan: Plan, cur: ActView, H: int, W: int, device, dtype) -> None:
        """Everything of the trunk + RPN plan behind net_conv = `cur`."""
        A, mk = self._num_anchors, dict(dtype=dtype, device=device)
        if cur.H < 2 or cur.W < 2:
            raise FlowtrackHipError(f"blob {H}x{W}: the {cur.H}x{cur.W} feature map is too small for the RoI crop (2x2 at least)")
        plan.net_conv = cur
        h, w = cur.H, cur.W
        # RPN (nets/network.py:227-244): 3x3 + bias + ReLU, then both 1x1 heads as one GEMM: channels [0, 2A) scores, [2A, 6A) deltas
        rpn = self.fused("rpn_net", self.rpn_net.weight, pad=1, bias=self.rpn_net.bias, act="relu", **mk)
        a_rpn = new_act(1, h, w, RPN_CHANNELS, dtype, device)
        rpn.record(prog, cur, a_rpn)
        heads = self.fused("rpn_cls_score_net+rpn_bbox_pred_net", torch.cat((self.rpn_cls_score_net.weight, self.rpn_bbox_pred_net.weight), 0),
                           bias=torch.cat((self.rpn_cls_score_net.bias, self.rpn_bbox_pred_net.bias), 0), act=None, **mk)
        a_out = new_act(1, h, w, 6 * A, dtype, device)
        heads.record(prog, a_rpn, a_out)
        code = _lib.dtype_code(dtype)
        plan.rpn_cls_score = torch.zeros((1, h, w, 2 * A), dtype=torch.float32, device=device)
        plan.rpn_bbox_pred = torch.zeros((1, h, w, 4 * A), dtype=torch.float32, device=device)
        plan.rpn_cls_prob = torch.zeros((1, h, w, 2 * A), dtype=torch.float32, device=device)
        # the fp32 [h*w, C] copies the proposal layer reads: NHWC channel windows as "NCHW" of h*w images of one pixel
        prog.add("ft_unpack_nhwc_to_nchw", a_out.t.data_ptr(), plan.rpn_cls_score.data_ptr(), h * w, 2 * A, 1, 1, a_out.cstride, 0, code,
                 keep=(a_out.t, plan.rpn_cls_score))
        prog.add("ft_unpack_nhwc_to_nchw", a_out.t.data_ptr(), plan.rpn_bbox_pred.data_ptr(), h * w, 4 * A, 1, 1, a_out.cstride, 2 * A, code,
                 keep=(a_out.t, plan.rpn_bbox_pred))
        prog.add("ft_rpn_softmax_fwd", code, a_out.t.data_ptr(), ctypes.c_longlong(h * w), A, a_out.cstride, 0, plan.rpn_cls_prob.data_ptr(),
                 keep=(a_out.t, plan.rpn_cls_prob))
        anchors, _ = proposal.generate_anchors_pre(h, w, FEAT_STRIDE, self._anchor_scales, self._anchor_ratios)
        plan.anchors = torch.from_numpy(anchors).to(device)

    def _record_crop(self, prog, plan: Plan, feat: ActView, rows: int, max_pool: bool, device, dtype) -> ActView:
        """_crop_pool_layer (nets/network.py:93-121) at `rows` RoIs: plan.rois [rows,5] -> plan.pool5 [rows,7,7,C]."""
        plan.rois = torch.zeros((rows, 5), dtype=torch.float32, device=device)
        pool5 = plan.pool5 = new_act(rows, proposal.POOLING_SIZE, proposal.POOLING_SIZE, feat.C, dtype, device)
        if feat.cstride != feat.C or pool5.cstride != feat.C:
            raise FlowtrackHipError("the RoI crop works on dense NHWC buffers")
        prog.add("ft_roi_crop_nhwc_fwd", _lib.dtype_code(dtype), feat.t.data_ptr(), plan.rois.data_ptr(), 1, feat.H, feat.W, feat.C, rows,
                 ctypes.c_float(FEAT_STRIDE), proposal.POOLING_SIZE, int(max_pool), pool5.t.data_ptr(), keep=(feat.t, plan.rois, pool5.t))
        return pool5

    def _record_cls_bbox(self, prog, plan: Plan, fc7: ActView, rows: int, device, dtype) -> None:
        """cls_score_net and bbox_pred_net as one GEMM on fc7 [rows,1,1,_fc7_channels] -> plan.fc_out fp32 [rows, 5 K]."""
        K = self._num_classes
        fc = self.fused("cls_score_net+bbox_pred_net", torch.cat((self.cls_score_net.weight, self.bbox_pred_net.weight), 0)[:, :, None, None],
                        bias=torch.cat((self.cls_score_net.bias, self.bbox_pred_net.bias), 0), act=None, dtype=dtype, device=device)
        plan.fc_out = torch.zeros((rows, 5 * K, 1, 1), dtype=torch.float32, device=device)
        fc.record(prog, fc7, plan.fc_out)

    def _build_trunk(self, H: int, W: int, device, dtype) -> Plan:
        prog = Program(self._side_stream(device))
        plan = Plan(prog, dtype=dtype, device=device, fallbacks=[], heads={})         # heads: rows -> the region-head plan
        plan.x_static = torch.zeros((1, 3, H, W), dtype=torch.float32, device=device)
        cur = self._record_trunk(prog, plan, H, W, device, dtype)
        self._record_rpn(prog, plan, cur, H, W, device, dtype)
        return plan

    def _build_head(self, trunk: Plan, rows: int, device, dtype) -> Plan:
        prog = Program(self._side_stream(device))
        plan = Plan(prog, fallbacks=[])
        fc7 = plan.fc7 = self._record_tail(prog, plan, trunk.net_conv, rows, device, dtype)
        self._record_cls_bbox(prog, plan, fc7, rows, device, dtype)
        return plan

    # -- plans -----------------------------------------------------------------------------------------------------------------
    def trunk_plan(self, H: int, W: int) -> Plan:
        """The trunk + RPN plan of one blob shape (and the current dtype / recording switches); its x_static [1,3,H,W] fp32 is the
        staged input ft_detect_blob_fwd writes."""
        if not hasattr(self, "rpn_net"):
            raise FlowtrackHipError("call create_architecture() first")
        device, dtype = self._resolve()
        key = (int(H), int(W), device, dtype) + tuple(self._plan_switches())
        return self._cached_plan(key, lambda: self._build_trunk(int(H), int(W), device, dtype))

    def head_plan(self, trunk: Plan, rows: int) -> Plan:
        return self._cached_plan(rows, lambda: self._build_head(trunk, rows, trunk.device, trunk.dtype), trunk.heads)

    # -- inference -------------------------------------------------------------------------------------------------------------
    def _stage(self, image) -> Plan:
        """image: the reference's blob, [1,H,W,3] fp32 (numpy or tensor) -> its plan with x_static filled."""
        t = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image
        if t.dim() != 4 or t.shape[0] != 1 or t.shape[3] != 3:
            raise FlowtrackHipError(f"expected a [1,H,W,3] blob (single image, as model/test.py:90), got {tuple(t.shape)}")
        plan = self.trunk_plan(t.shape[1], t.shape[2])
        plan.x_static.copy_(t.to(plan.x_static.device).permute(0, 3, 1, 2))
        return plan

    @torch.no_grad()
    def detect_staged(self, plan: Plan, im_info, frame_shape=None, keep_intermediates: bool = False) -> dict:
        """Everything behind the staged input: fills and returns self._predictions (device tensors, fp32, the reference's layouts).
        frame_shape (h, w) of the original frame adds `pred_boxes` [R,4K] (model/test.py:97-104)."""
        self._check_eval()
        K, A = self._num_classes, self._num_anchors
        im_info = [float(v) for v in np.asarray(im_info, dtype=np.float64).reshape(-1)[:3]]
        self.run(plan)
        rois, _ = proposal.proposal_layer(plan.rpn_cls_prob, plan.rpn_bbox_pred, im_info, "TEST", self._feat_stride[0], plan.anchors, A,
                                          pre_nms_topN=self.rpn_pre_nms_topN, post_nms_topN=self.rpn_post_nms_topN,
                                          nms_thresh=self.rpn_nms_thresh)
        p = self._predictions = {"rpn_cls_score": plan.rpn_cls_score.clone(), "rpn_cls_prob": plan.rpn_cls_prob.clone(),
                                 "rpn_bbox_pred": plan.rpn_bbox_pred.clone(), "rois": rois}
        if keep_intermediates:
            p["net_conv"] = plan.net_conv.t[..., :plan.net_conv.C].permute(0, 3, 1, 2).float().contiguous()
        p.update(self.region_head(plan, rois, im_info[2], frame_shape, keep_intermediates))
        return p

    @torch.no_grad()
    def region_head(self, plan: Plan, rois: torch.Tensor, im_scale: float = 1.0, frame_shape=None, keep_intermediates: bool = False) -> dict:
        """The region head on `rois` [n,5] (blob pixels) against the plan's current net_conv: cls_score, cls_pred, cls_prob and the
        un-normalised bbox_pred, (+ pred_boxes with frame_shape, + pool5 / fc7 with keep_intermediates)."""
        K = self._num_classes
        device = plan.device
        n = int(rois.shape[0])
        rows = max(RPN_POST_DEFAULT if self.rpn_post_nms_topN is None else int(self.rpn_post_nms_topN), n, 1)
        hp = self.head_plan(plan, rows)
        hp.rois.zero_()
        hp.rois[:n].copy_(rois)
        self.run(hp)
        fc = hp.fc_out.view(rows, 5 * K)
        out = {"cls_score": fc[:n, :K].contiguous(), "bbox_pred": torch.empty((n, 4 * K), dtype=torch.float32, device=device),
               "cls_prob": torch.empty((n, K), dtype=torch.float32, device=device)}
        raw = fc[:n, K:].contiguous()
        boxes = torch.empty((n, 4 * K), dtype=torch.float32, device=device) if frame_shape is not None else None
        fh, fw = (float(frame_shape[0]), float(frame_shape[1])) if frame_shape is not None else (1.0, 1.0)
        rois_c = rois.contiguous()
        with torch.cuda.device(device):
            check(_lib.load().ft_rcnn_detections_fwd(out["cls_score"].data_ptr(), raw.data_ptr(), rois_c.data_ptr(), n, K,
                                                     (ctypes.c_float * 4)(*BBOX_NORMALIZE_STDS), (ctypes.c_float * 4)(*BBOX_NORMALIZE_MEANS),
                                                     float(im_scale), fh, fw, out["cls_prob"].data_ptr(), out["bbox_pred"].data_ptr(),
                                                     boxes.data_ptr() if boxes is not None else None, current_stream_handle(device)),
                  "ft_rcnn_detections_fwd")
        out["cls_pred"] = out["cls_score"].argmax(1) if n else torch.empty(0, dtype=torch.long, device=device)
        if boxes is not None:
            out["pred_boxes"] = boxes
        if keep_intermediates:
            out["pool5"] = hp.pool5.t[:n].permute(0, 3, 1, 2).float().contiguous()
            out["fc7"] = hp.fc7.t[:n, 0, 0, :].float().contiguous()
        return out

    @torch.no_grad()
    def detect_enqueue(self, plan: Plan, im_info, frame_shape, out_slot, person_id: int = 1, thresh: float = 0.3, min_score: float = 0.0,
                       extra=None, extra_count=None, max_keep: int = 0) -> None:
        """detect_staged + the person NMS of detection.test.detect_persons for the staged frame, enqueued on the current stream with
        nothing read from the device: the trunk plan, proposal.proposal_layer_device into the head plan's rois at rows =
        post_nms_topN (the row count region_head uses whenever n <= post_nms_topN: both paths replay the identical head plan), the
        head plan, ft_rcnn_detections_fwd over all rows (rows past the kept count come from zero RoIs; ft_detect_select_fwd masks
        them), ft_detect_select_fwd into out_slot = (dets fp32 [cap,5], count int32 [1]), both CUDA tensors (views of a clip's
        buffers).  extra: fp32 CUDA [M,5] boxes that join the NMS (extra_count: int32 [1] on the device, all M rows without it).
        self._predictions is not touched.  A plan's first run builds and captures it (HipModule.run): that one call waits."""
        self._check_eval()
        K, A = self._num_classes, self._num_anchors
        device = plan.device
        im_info = [float(v) for v in np.asarray(im_info, dtype=np.float64).reshape(-1)[:3]]
        dets, count = out_slot
        for t, dt, what in ((dets, torch.float32, "dets [cap,5]"), (count, torch.int32, "count [1]")):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != device or not t.is_contiguous():
                raise FlowtrackHipError(f"detect_enqueue out_slot: {what} is a contiguous {dt} tensor on {device}")
        if dets.dim() != 2 or dets.shape[1] != 5 or dets.shape[0] < 1 or count.numel() != 1:
            raise FlowtrackHipError(f"detect_enqueue out_slot: expected (dets [cap,5], count [1]), got {tuple(dets.shape)}, {tuple(count.shape)}")
        M = 0
        if extra is not None:
            if not isinstance(extra, torch.Tensor) or extra.dtype != torch.float32 or extra.device != device or extra.dim() != 2 or \
                    extra.shape[1] != 5 or not extra.is_contiguous():
                raise FlowtrackHipError("detect_enqueue extra: expected a contiguous fp32 [M,5] tensor on the net's device")
            M = int(extra.shape[0])
            if M == 0:
                extra = None
        rows = max(RPN_POST_DEFAULT if self.rpn_post_nms_topN is None else int(self.rpn_post_nms_topN), 1)
        self.run(plan)
        hp = self.head_plan(plan, rows)
        _, n_rois = proposal.proposal_layer_device(plan.rpn_cls_prob, plan.rpn_bbox_pred, im_info, "TEST", self._feat_stride[0], plan.anchors, A,
                                                   hp.rois, pre_nms_topN=self.rpn_pre_nms_topN, post_nms_topN=self.rpn_post_nms_topN,
                                                   nms_thresh=self.rpn_nms_thresh)
        self.run(hp)
        fc = hp.fc_out.view(rows, 5 * K)
        cls_score, raw = fc[:, :K].contiguous(), fc[:, K:].contiguous()
        cls_prob = torch.empty((rows, K), dtype=torch.float32, device=device)
        boxes = torch.empty((rows, 4 * K), dtype=torch.float32, device=device)
        lib = _lib.load()
        with torch.cuda.device(device):
            stream = current_stream_handle(device)
            check(lib.ft_rcnn_detections_fwd(cls_score.data_ptr(), raw.data_ptr(), hp.rois.data_ptr(), rows, K,
                                             (ctypes.c_float * 4)(*BBOX_NORMALIZE_STDS), (ctypes.c_float * 4)(*BBOX_NORMALIZE_MEANS),
                                             im_info[2], float(frame_shape[0]), float(frame_shape[1]), cls_prob.data_ptr(), None,
                                             boxes.data_ptr(), stream), "ft_rcnn_detections_fwd")
            check(lib.ft_detect_select_fwd(cls_prob.data_ptr(), boxes.data_ptr(), rows, n_rois.data_ptr(), K, int(person_id),
                                           extra.data_ptr() if extra is not None else None, M,
                                           extra_count.data_ptr() if extra_count is not None else None, float(min_score), float(thresh),
                                           int(max_keep), int(dets.shape[0]), dets.data_ptr(), count.data_ptr(), stream),
                  "ft_detect_select_fwd")

    def forward(self, image, im_info, gt_boxes=None, mode="TRAIN", keep_intermediates: bool = False):
        if mode != "TEST" or gt_boxes is not None:
            raise FlowtrackHipError(f"{type(self).__name__}: only mode='TEST' without gt_boxes runs on the HIP path (targets and losses are out of scope)")
        self.detect_staged(self._stage(image), im_info, None, keep_intermediates)

    def test_image(self, image, im_info, keep_intermediates: bool = False):
        """nets/network.py:418-425: (cls_score [R,K], cls_prob [R,K], bbox_pred [R,4K], rois [R,5]) as numpy."""
        self.eval()
        self.forward(image, im_info, None, mode="TEST", keep_intermediates=keep_intermediates)
        p = self._predictions
        return tuple(p[k].cpu().numpy() for k in ("cls_score", "cls_prob", "bbox_pred", "rois"))

    @torch.no_grad()
    def extract_head(self, image) -> torch.Tensor:
        """nets/network.py:413-415: net_conv [1,_net_conv_channels,h,w] fp32 of a [1,H,W,3] blob."""
        self._check_eval()
        plan = self._stage(image)
        self.run(plan)
        return plan.net_conv.t[..., :plan.net_conv.C].permute(0, 3, 1, 2).float().contiguous()

    # -- what the HIP path does not have ---------------------------------------------------------------------------------------
    def _no_training(self, *a, **k):
        raise FlowtrackHipError(f"{type(self).__name__}: training steps, losses and summaries are out of scope on the HIP path")

    train_step = train_step_with_summary = train_step_no_return = get_summary = _add_losses = _no_training

    def delete_intermediate_states(self):
        self._predictions = {}


class resnetv1(_FasterRCNN):
    #: fold each block-0 projection shortcut into its conv3 launch (FusedShortcutConv); FT_FUSE_SHORTCUT=0 / False keeps them apart
    fuse_shortcut: bool = os.environ.get("FT_FUSE_SHORTCUT", "1") != "0"
    #: identity blocks as one launch where the library takes the shape, recorded as a choice next to the three convs (the first-call
    #: benchmark keeps one); FT_FUSE_BOTTLENECK=0 / False keeps three convs, "force" records the one-launch form alone (dev, tests)
    fuse_bottleneck = os.environ.get("FT_FUSE_BOTTLENECK", "1") != "0"

    def __init__(self, num_layers: int = 50):
        super().__init__()
        self._num_layers = num_layers
        self._net_conv_channels = 1024
        self._fc7_channels = 2048

    # -- construction (nets/resnet_v1.py:116-129) --------------------------------------------------------------------------------
    def _init_head_tail(self):
        if self._num_layers not in BLOCKS:
            raise NotImplementedError      # other depths are not supported, as in the reference
        self.resnet = _ResNet(BLOCKS[self._num_layers])

    def load_pretrained_cnn(self, state_dict):
        self.resnet.load_state_dict({k: state_dict[k] for k in list(self.resnet.state_dict())})
        self._invalidate()

    def _plan_switches(self):
        return bool(self.fuse_shortcut), self.fuse_bottleneck

    # -- recording -------------------------------------------------------------------------------------------------------------
    def _record_layer(self, prog, li: int, cur: ActView, fallbacks: list) -> ActView:
        """One stage of Caffe-strided Bottlenecks (conv1 and the shortcut carry the stride, nets/resnet_v1.py:30-35) in the forms this
        host offers: the identity block's one-launch form (alone with fuse_bottleneck = "force"), the shortcut GEMM behind its query,
        plain launches.  `fallbacks` collects the blocks recorded as plain launches where a fused form was offered."""
        forms = ((("fused-only" if self.fuse_bottleneck == "force" else "fused"),) if self.fuse_bottleneck else ()) + \
            (("shortcut-asked",) if self.fuse_shortcut else ())
        for bi, blk in enumerate(getattr(self.resnet, f"layer{li}")):
            stride = 2 if (bi == 0 and li in (2, 3)) else 1          # layer4.0 has stride 1 throughout (resnet_v1.py:33-35)
            cur = record_block(self, prog, f"resnet.layer{li}.{bi}", blk, cur, stride=stride, stride_on="conv1", forms=forms, fallbacks=fallbacks)
        return cur

    def _record_trunk(self, prog, plan: Plan, H: int, W: int, device, dtype) -> ActView:
        mk = dict(dtype=dtype, device=device)
        a_in = new_rowpacked_act(1, H, W, 3, 3, dtype, device)
        record_pack_input(prog, plan.x_static, a_in)
        r = self.resnet
        stem = self.fused("resnet.conv1", r.conv1.weight, stride=2, pad=3, bn=r.bn1.as_dict(), act="relu", **mk)
        H1, W1 = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
        a1 = new_act(1, H1, W1, 64, dtype, device)
        stem.record(prog, a_in, a1)
        cur = new_act(1, conv_out(H1, 3, 2, 1), conv_out(W1, 3, 2, 1), 64, dtype, device)
        record_maxpool(prog, a1, cur)
        for li in (1, 2, 3):
            cur = self._record_layer(prog, li, cur, plan.fallbacks)
        return cur

    def _record_tail(self, prog, plan: Plan, feat: ActView, rows: int, device, dtype) -> ActView:
        pool5 = self._record_crop(prog, plan, feat, rows, False, device, dtype)
        cur = self._record_layer(prog, 4, pool5, plan.fallbacks)
        if cur.cstride != cur.C:
            raise FlowtrackHipError("the mean pool works on dense NHWC buffers")
        plan.layer4 = cur
        fc7 = new_act(rows, 1, 1, cur.C, dtype, device)
        prog.add("ft_rcnn_mean_pool_fwd", _lib.dtype_code(dtype), cur.t.data_ptr(), rows, cur.H, cur.C, fc7.t.data_ptr(), keep=(cur.t, fc7.t))
        return fc7


class vgg16(_FasterRCNN):
    #: how classifier.0 / .3 are recorded in fp16: "" records both forms as a choice (the first-call benchmark keeps one; without a
    #: benchmark the first recorded, FC_FIRST, runs), "fc" records ft_fc_fwd alone, "igemm" ft_conv2d_fwd alone (dev, tests).
    #: fp32 always records "igemm".  FT_VGG_FC sets the default.
    fc_form: str = os.environ.get("FT_VGG_FC", "")
    #: the recorder's first option of that choice: the form the measurement at rows = 300 favours (profiles/README.md, "VGG16
    #: detector": igemm 115 / 33 us against fc 138 / 38 us for classifier.0 / .3)
    FC_FIRST = "igemm"

    def __init__(self):
        super().__init__()
        self._net_conv_channels = 512
        self._fc7_channels = 4096

    # -- construction (nets/vgg16.py:28-38, :52-53) ------------------------------------------------------------------------------
    def _init_head_tail(self):
        self.vgg = _VGG()

    def load_pretrained_cnn(self, state_dict):
        """The keys of `vgg` that `state_dict` has: an ImageNet dict with classifier.6.* loads (nets/vgg16.py:52-53)."""
        own = self.vgg.state_dict()
        own.update({k: v for k, v in state_dict.items() if k in own})
        self.vgg.load_state_dict(own)
        self._invalidate()

    def _plan_switches(self):
        if self.fc_form not in ("", "fc", "igemm"):
            raise FlowtrackHipError(f"vgg16.fc_form is '', 'fc' or 'igemm', not {self.fc_form!r}")
        return (self.fc_form,)

    # -- recording -------------------------------------------------------------------------------------------------------------
    def _record_trunk(self, prog, plan: Plan, H: int, W: int, device, dtype) -> ActView:
        """nets/vgg16.py:38: features[:-1].  Every conv is 3x3 / pad 1 + bias + ReLU (the epilogue of ft_conv2d_fwd); the first one
        (Cin = 3) reads the row-packed input, as the ResNet stem does."""
        mk = dict(dtype=dtype, device=device)
        cur = new_rowpacked_act(1, H, W, 3, 1, dtype, device)
        record_pack_input(prog, plan.x_static, cur)
        mods = list(self.vgg.features)[:-1]
        for i, m in enumerate(mods):
            if isinstance(m, ConvParams):
                conv = self.fused(f"vgg.features.{i}", m.weight, pad=1, bias=m.bias, act="relu", **mk)
                nxt = new_act(1, cur.H, cur.W, m.cout, dtype, device)
                conv.record(prog, cur, nxt)
                cur = nxt
            elif m.kind == "maxpool2x2s2":
                if cur.H < 2 or cur.W < 2:
                    raise FlowtrackHipError(f"blob {H}x{W}: the {cur.H}x{cur.W} map in front of vgg.features.{i} is too small to pool")
                nxt = new_act(1, cur.H // 2, cur.W // 2, cur.C, dtype, device)
                record_maxpool2x2(prog, cur, nxt)
                cur = nxt
        return cur

    def _fc6_weight(self) -> torch.Tensor:
        """classifier.0.weight [4096, 512*7*7] is laid out over (c, h, w) (nets/vgg16.py:47: pool5.view(R, -1) of an NCHW tensor);
        the pooled buffer here is (h, w, c)."""
        w = self.vgg.classifier[0].weight
        P = proposal.POOLING_SIZE
        return w.detach().view(w.shape[0], self._net_conv_channels, P, P).permute(0, 2, 3, 1).reshape(w.shape[0], -1)

    def _record_fc(self, prog, label: str, weight: torch.Tensor, bias: torch.Tensor, x: ActView, y: ActView, device, dtype) -> None:
        """One classifier layer + ReLU, [rows,1,1,K] -> [rows,1,1,N], in the forms fc_form allows."""
        rows, (n, k) = x.N, weight.shape
        only = "igemm" if dtype != torch.float16 else self.fc_form or None
        if only != "igemm" and not FusedFC.supported(rows, k, n, dtype, x, y):
            raise FlowtrackHipError(f"{label}: ft_fc_fwd does not take {rows} rows of [{n}, {k}]")
        forms = {"fc": lambda: self._cached(label + "|fc", dtype, device, lambda: FusedFC(weight, bias, device=device, act="relu", label=label)).record(prog, x, y),
                 "igemm": lambda: self.fused(label, weight[:, :, None, None], bias=bias, act="relu", dtype=dtype, device=device).record(prog, x, y)}
        prog.choice(f"fc|{rows}x{k}x{n}", {form: forms[form] for form in sorted(forms, key=lambda f: f != self.FC_FIRST)}, only=only)

    def _record_tail(self, prog, plan: Plan, feat: ActView, rows: int, device, dtype) -> ActView:
        """nets/vgg16.py:46-50: pool5.view(R, -1) -> classifier (Linear, ReLU, Dropout, Linear, ReLU, Dropout), in eval."""
        pool5 = self._record_crop(prog, plan, feat, rows, True, device, dtype)
        c = self.vgg.classifier
        x6 = ActView(pool5.t.view(rows, 1, 1, -1), c[0].cin)
        fc6 = plan.fc6 = new_act(rows, 1, 1, c[0].cout, dtype, device)
        self._record_fc(prog, "vgg.classifier.0", self._fc6_weight(), c[0].bias, x6, fc6, device, dtype)
        fc7 = new_act(rows, 1, 1, c[3].cout, dtype, device)
        self._record_fc(prog, "vgg.classifier.3", c[3].weight, c[3].bias, fc6, fc7, device, dtype)
        return fc7


RPN_POST_DEFAULT = proposal.RPN_DEFAULTS["TEST"][1]
