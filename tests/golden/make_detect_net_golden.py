#!/usr/bin/env python3
"""Generates tests/golden/detect_net_golden.npz by importing and running the ORIGINAL reference's detector on the CPU:
lib/detection/nets/resnet_v1.py: resnetv1, nets/network.py: Network and model/test.py: im_detect.  Like make_detect_golden.py it
needs the reference checkout, so nothing in tests/, bench.py or smoke() ever runs this file; they only read the .npz it wrote.

The reference's import chain asks for modules that are not installed here or that bind CUDA-only extensions.  They are replaced
before it is imported, by stand-ins that hold no reference text:
  easydict                                   a dict with attribute access
  tensorboardX, scipy.misc.imresize, utils.visualization, utils.bbox      empty stand-ins (training / summaries only)
  torchvision.models.resnet                  this file's restatement of torchvision 0.2's ResNet / Bottleneck / BasicBlock
  model.nms_wrapper.nms                      tests/detect_ref.nms(inclusive=False): the CUDA rule the reference's detector runs
  layer_utils.roi_pooling.roi_pool           a stand-in that refuses to run (POOLING_MODE is 'crop')
  layer_utils.roi_align.crop_and_resize      CropAndResizeFunction on tests/detect_ref.crop_and_resize (fp32)
  cv2                                        resize = tests/detect_net_ref.resize_linear in float64 (OpenCV's INTER_LINEAR rule for float
                                             images), cast to float32; parity with OpenCV itself is therefore NOT pinned by this file
  torch.Tensor.cuda                          identity
  a forward hook on rpn_cls_score_net        makes its output contiguous (the `.view` at network.py:234 otherwise fails on the CPU)

Weights: synth.fill_detector_state_dict(seed); frames: synth.detector_frame(seed, H, W); neither is stored.  Two cases, both
ResNet-50, num_classes 3, person_id 1, TEST.SCALES (75,), TEST.MAX_SIZE 125:
  a   50 x 72 frame, scale 1.5, blob 75 x 108
  b   40 x 96 frame, the MAX_SIZE branch (125 / 96), blob 52 x 125
Stored per case (prefix a_ / b_): blob, im_info, net_conv, rpn_cls_score, rpn_cls_prob, rpn_bbox_pred, rois, cls_score, cls_prob,
bbox_pred, scores, pred_boxes, persons (lib/tracking/net_utils.py: detect's steps on the reference's scores and boxes, with the
stand-in NMS); plus seed, frame_hw / target_size / max_size, and the state_dict keys and shapes of depths 50 and 101.

The seed is the first from SEED0 upwards at which, in BOTH cases and from the reference's own run: max |net_conv| <= 32; at least
a quarter of the foreground probabilities and of the person probabilities lie in (0.1, 0.9); |rpn_bbox_pred| <= 1 and |bbox_pred|
<= 1; at least 8 RoIs are kept and the RPN NMS drops at least one box; the person NMS keeps at least 2 boxes and suppresses at least
1; and tests/detect_net_ref.py reproduces every stored continuous tensor to 1e-5.  The script aborts rather than write a file that
fails one.  The file is written with fixed zip timestamps: it regenerates byte-equal.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import detect_net_ref  # noqa: E402
import detect_ref  # noqa: E402
from make_detect_golden import _AttrDict, save_npz  # noqa: E402
from flowtrack.pytorch_amd import synth  # noqa: E402

SEED0 = 20261020
NUM_CLASSES, PERSON_ID = 3, 1
TARGET, MAX_SIZE = 75, 125
CASES = {"a": (50, 72), "b": (40, 96)}
RESTATEMENT_TOL = 1e-5
CONTINUOUS = ("blob", "net_conv", "rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "rois", "cls_score", "cls_prob", "bbox_pred", "scores",
              "pred_boxes")


# ---- torchvision 0.2's resnet, restated ---------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000):
        self.inplanes = 64
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], 2)
        self.avgpool = nn.AvgPool2d(7, stride=1)
        self.fc = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        mods = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        mods += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*mods)


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _CropAndResize:
    def __init__(self, crop_height, crop_width, extrapolation_value=0):
        self.ch, self.cw, self.ext = int(crop_height), int(crop_width), float(extrapolation_value)

    def __call__(self, image, boxes, box_ind):
        return torch.from_numpy(detect_ref.crop_and_resize(image.detach().numpy(), boxes.detach().numpy(), box_ind.numpy(), self.ch, self.cw, self.ext))


class _NoRoIPool:
    def __init__(self, *a, **k):
        raise RuntimeError("the golden runs POOLING_MODE = 'crop'")


def _cv2_resize(src, dsize=None, dst=None, fx=0, fy=0, interpolation=1):
    assert dsize is None and interpolation == 1 and src.dtype == np.float32
    H, W = src.shape[:2]
    Hb, Wb = int(np.rint(H * fy)), int(np.rint(W * fx))
    return detect_net_ref.resize_linear(src, Hb, Wb, 1.0 / fy, 1.0 / fx, np.float64).astype(np.float32)


def import_reference():
    _module("easydict", EasyDict=_AttrDict)
    _module("tensorboardX")
    if "scipy" not in sys.modules:
        try:
            import scipy  # noqa: F401
        except ImportError:
            _module("scipy")
    _module("scipy.misc", imresize=None)
    _module("cv2", resize=_cv2_resize, INTER_LINEAR=1)
    tv_resnet = _module("torchvision.models.resnet", ResNet=ResNet, Bottleneck=Bottleneck, BasicBlock=BasicBlock)
    tv_models = _module("torchvision.models", resnet=tv_resnet)
    _module("torchvision", models=tv_models)
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REF, "lib", "detection"))
    import layer_utils  # noqa: F401  (the reference's packages)
    import model  # noqa: F401
    import utils  # noqa: F401
    _module("utils.visualization", draw_bounding_boxes=None)
    _module("utils.bbox", bbox_overlaps=None)
    _module("model.nms_wrapper",
            nms=lambda dets, thresh: torch.from_numpy(detect_ref.nms(dets.detach().numpy(), thresh, inclusive=False).astype(np.int64)))
    _module("layer_utils.roi_pooling")
    _module("layer_utils.roi_pooling.roi_pool", RoIPoolFunction=_NoRoIPool)
    _module("layer_utils.roi_align")
    _module("layer_utils.roi_align.crop_and_resize", CropAndResizeFunction=_CropAndResize)
    from model import test as ref_test
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    return resnetv1, ref_test, cfg


def shapes_of(net):
    keys = list(net.state_dict())
    return np.array(keys), np.array([";".join(str(d) for d in net.state_dict()[k].shape) for k in keys])


def run_case(net, ref_test, frame):
    """The reference's im_detect on `frame` and every seam it leaves in net._predictions, as numpy."""
    seams = {}
    handle = net._layers["head"].register_forward_hook(lambda m, i, o: seams.__setitem__("net_conv", o.detach().numpy().copy()))
    blob, scales = ref_test._get_blobs(frame)
    with torch.no_grad():
        scores, pred_boxes = ref_test.im_detect(net, frame)
    handle.remove()
    p = net._predictions
    out = {k: p[k].detach().numpy().copy() for k in ("rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "rois", "cls_score", "cls_prob", "bbox_pred")}
    out.update(seams, blob=blob["data"].transpose(0, 3, 1, 2).copy(), scores=np.asarray(scores), pred_boxes=np.asarray(pred_boxes),
               im_info=np.array([blob["data"].shape[1], blob["data"].shape[2], scales[0]], dtype=np.float32))
    return out


def conditions(o, persons):
    fg = o["rpn_cls_prob"][..., o["rpn_cls_prob"].shape[-1] // 2:]
    pp = o["cls_prob"][:, PERSON_ID]
    return {"max |net_conv| <= 32": np.abs(o["net_conv"]).max() <= 32,
            "a quarter of the foreground probabilities in (0.1, 0.9)": ((fg > 0.1) & (fg < 0.9)).mean() >= 0.25,
            "|rpn_bbox_pred| <= 1": np.abs(o["rpn_bbox_pred"]).max() <= 1,
            "at least 8 RoIs, at least one box dropped by the RPN NMS": 8 <= len(o["rois"]) < min(fg.size, 300),
            "a quarter of the person probabilities in (0.1, 0.9)": ((pp > 0.1) & (pp < 0.9)).mean() >= 0.25,
            "|bbox_pred| <= 1": np.abs(o["bbox_pred"]).max() <= 1,
            "the person NMS keeps >= 2 and suppresses >= 1": 2 <= len(persons) < len(o["rois"])}


def restatement_errors(sd, frame, o):
    mine = detect_net_ref.im_detect(sd, frame, 50, TARGET, MAX_SIZE)
    errs = {}
    for k in CONTINUOUS:
        errs[k] = float(np.abs(np.asarray(mine[k], dtype=np.float64) - np.asarray(o[k], dtype=np.float64)).max()) \
            if np.shape(mine[k]) == np.shape(o[k]) else float("inf")
    return errs


def main():
    resnetv1, ref_test, cfg = import_reference()
    cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = (TARGET,), MAX_SIZE
    assert cfg.POOLING_MODE == "crop" and not cfg.RESNET.MAX_POOL and cfg.TEST.MODE == "nms" and cfg.TEST.BBOX_REG
    out = {}
    for depth in (50, 101):
        net = resnetv1(depth)
        net.create_architecture(NUM_CLASSES, tag="default")
        out[f"keys_{depth}"], out[f"shapes_{depth}"] = shapes_of(net)
    net = resnetv1(50)
    net.create_architecture(NUM_CLASSES, tag="default")
    net.rpn_cls_score_net.register_forward_hook(lambda m, i, o: o.contiguous())
    net.eval()
    seed = SEED0
    while True:
        sd = synth.fill_detector_state_dict(net.state_dict(), seed)
        net.load_state_dict(sd)
        results, ok = {}, True
        for name, (H, W) in CASES.items():
            frame = synth.detector_frame(seed, H, W)
            o = run_case(net, ref_test, frame)
            o["persons"] = detect_net_ref.detect_persons(o["scores"], o["pred_boxes"], PERSON_ID, 0.3)
            conds = conditions(o, o["persons"])
            results[name] = (frame, o, conds)
            ok = ok and all(conds.values())
        if ok or seed >= SEED0 + 64:
            break
        seed += 1
    for name, (frame, o, conds) in results.items():
        for what, held in conds.items():
            assert held, f"seed {seed}, case {name}: {what} does not hold"
        errs = restatement_errors(sd, frame, o)
        print(f"case {name}: blob {o['blob'].shape[2:]}, net_conv {o['net_conv'].shape[2:]} max {np.abs(o['net_conv']).max():.2f}, "
              f"{len(o['rois'])} RoIs, {len(o['persons'])} persons; restatement errors " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= RESTATEMENT_TOL, f"case {name}: tests/detect_net_ref.py misses the reference's {k} by {v}"
        out.update({f"{name}_{k}": v for k, v in o.items()})
        out[f"{name}_frame_hw"] = np.array(frame.shape[:2], dtype=np.int32)
    out.update(seed=np.int64(seed), target_size=np.int32(TARGET), max_size=np.int32(MAX_SIZE), num_classes=np.int32(NUM_CLASSES),
               person_id=np.int32(PERSON_ID))
    path = os.path.join(HERE, "detect_net_golden.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
