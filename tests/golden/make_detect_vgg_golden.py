#!/usr/bin/env python3
"""Generates tests/golden/detect_vgg_golden.npz by importing and running the ORIGINAL reference's VGG16 detector on the CPU:
lib/detection/nets/vgg16.py: vgg16, nets/network.py: Network and model/test.py: im_detect.  It works the way
make_detect_net_golden.py does and imports that file's stand-ins (easydict, tensorboardX, cv2.resize, the NMS, crop_and_resize, ...);
like it, it needs the reference checkout, so nothing in tests/, bench.py or smoke() ever runs this file; they only read the .npz.

One more stand-in, which holds no reference text: `torchvision.models.vgg16` is this file's restatement of torchvision 0.2's VGG
(config D, no BatchNorm: 13 convs + ReLU with five max-pools, and the three-layer classifier the reference cuts fc8 from).

Weights: synth.fill_vgg_detector_state_dict(seed); frames: synth.detector_frame(seed, H, W); neither is stored.  The two cases of
make_detect_net_golden.py, num_classes 3, person_id 1, TEST.SCALES (75,), TEST.MAX_SIZE 125:
  a   50 x 72 frame, scale 1.5, blob 75 x 108 -> net_conv 4 x 6   (pools meet the odd maps 37 x 54, 27, 9 x 13)
  b   40 x 96 frame, the MAX_SIZE branch (125 / 96), blob 52 x 125 -> net_conv 3 x 7   (odd maps 125, 13 x 31, 15)
Stored per case (prefix a_ / b_): what make_detect_net_golden.py stores, plus fc7 of the first FC7_ROWS RoIs; and seed, frame_hw /
target_size / max_size, the state_dict keys and shapes.

The seed is the first from SEED0 upwards at which, in BOTH cases and from the reference's own run, the conditions of
make_detect_net_golden.py hold (max |net_conv| <= 32; a quarter of the foreground and of the person probabilities in (0.1, 0.9);
|rpn_bbox_pred| <= 1 and |bbox_pred| <= 1; at least 8 RoIs with at least one box dropped by the RPN NMS; the person NMS keeps at
least 2 boxes and suppresses at least 1), max |fc7| <= 32 and all foreground scores are distinct (the reference's sort leaves the
order of a tie open); and tests/detect_vgg_ref.py reproduces every stored continuous tensor to 1e-5.  The script aborts rather than write a file that fails one.  Fixed zip timestamps: it regenerates byte-equal.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_detect_net_golden as base  # noqa: E402
import detect_net_ref  # noqa: E402
import detect_vgg_ref  # noqa: E402
from make_detect_golden import save_npz  # noqa: E402
from flowtrack.pytorch_amd import synth  # noqa: E402

SEED0 = 20261021
NUM_CLASSES, PERSON_ID, TARGET, MAX_SIZE, CASES = base.NUM_CLASSES, base.PERSON_ID, base.TARGET, base.MAX_SIZE, base.CASES
FC7_ROWS = 8
CONTINUOUS = base.CONTINUOUS + ("fc7",)
CFG_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


# ---- torchvision 0.2's vgg16, restated ------------------------------------------------------------------------------------------
class VGG(nn.Module):
    def __init__(self, features, num_classes=1000):
        super().__init__()
        self.features = features
        self.classifier = nn.Sequential(nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(True),
                                        nn.Dropout(), nn.Linear(4096, num_classes))

    def forward(self, x):
        x = self.features(x)
        return self.classifier(x.view(x.size(0), -1))


def vgg16(pretrained=False, **kw):
    assert not pretrained
    mods, cin = [], 3
    for v in CFG_D:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return VGG(nn.Sequential(*mods), **kw)


def import_reference():
    _, ref_test, cfg = base.import_reference()
    sys.modules["torchvision.models"].vgg16 = vgg16
    from nets.vgg16 import vgg16 as ref_vgg16
    return ref_vgg16, ref_test, cfg


def run_case(net, ref_test, frame):
    seams = {}
    handle = net.vgg.classifier.register_forward_hook(lambda m, i, o: seams.__setitem__("fc7", o.detach().numpy()[:FC7_ROWS].copy()))
    out = base.run_case(net, ref_test, frame)
    handle.remove()
    out.update(seams)
    return out


def restatement_errors(sd, frame, o):
    mine = detect_vgg_ref.im_detect(sd, frame, TARGET, MAX_SIZE)
    mine["fc7"] = mine["fc7"][:FC7_ROWS]
    errs = {}
    for k in CONTINUOUS:
        errs[k] = float(np.abs(np.asarray(mine[k], dtype=np.float64) - np.asarray(o[k], dtype=np.float64)).max()) \
            if np.shape(mine[k]) == np.shape(o[k]) else float("inf")
    return errs


def main():
    ref_vgg16, ref_test, cfg = import_reference()
    cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = (TARGET,), MAX_SIZE
    assert cfg.POOLING_MODE == "crop" and cfg.TEST.MODE == "nms" and cfg.TEST.BBOX_REG
    net = ref_vgg16()
    net.create_architecture(NUM_CLASSES, tag="default")
    out = {}
    out["keys"], out["shapes"] = base.shapes_of(net)
    net.rpn_cls_score_net.register_forward_hook(lambda m, i, o: o.contiguous())
    net.eval()
    seed = SEED0
    while True:
        sd = synth.fill_vgg_detector_state_dict(net.state_dict(), seed)
        net.load_state_dict(sd)
        results, ok = {}, True
        for name, (H, W) in CASES.items():
            frame = synth.detector_frame(seed, H, W)
            o = run_case(net, ref_test, frame)
            o["persons"] = detect_net_ref.detect_persons(o["scores"], o["pred_boxes"], PERSON_ID, 0.3)
            conds = base.conditions(o, o["persons"])
            conds["max |fc7| <= 32"] = np.abs(o["fc7"]).max() <= 32
            fg = o["rpn_cls_prob"][..., o["rpn_cls_prob"].shape[-1] // 2:]
            conds["all foreground scores distinct"] = np.unique(fg).size == fg.size      # (a tie is ordered by the sort's whim)
            results[name] = (frame, o, conds)
            ok = ok and all(conds.values())
            print(f"seed {seed} case {name}: " + ", ".join(f"{'ok' if v else 'NO'} {k}" for k, v in conds.items()), flush=True)
        if ok or seed >= SEED0 + 8:
            break
        seed += 1
    for name, (frame, o, conds) in results.items():
        for what, held in conds.items():
            assert held, f"seed {seed}, case {name}: {what} does not hold"
        errs = restatement_errors(sd, frame, o)
        print(f"case {name}: blob {o['blob'].shape[2:]}, net_conv {o['net_conv'].shape[2:]} max {np.abs(o['net_conv']).max():.2f}, "
              f"fc7 max {np.abs(o['fc7']).max():.2f}, {len(o['rois'])} RoIs, {len(o['persons'])} persons; restatement errors "
              + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= base.RESTATEMENT_TOL, f"case {name}: tests/detect_vgg_ref.py misses the reference's {k} by {v}"
        out.update({f"{name}_{k}": v for k, v in o.items()})
        out[f"{name}_frame_hw"] = np.array(frame.shape[:2], dtype=np.int32)
    out.update(seed=np.int64(seed), target_size=np.int32(TARGET), max_size=np.int32(MAX_SIZE), num_classes=np.int32(NUM_CLASSES),
               person_id=np.int32(PERSON_ID), fc7_rows=np.int32(FC7_ROWS))
    path = os.path.join(HERE, "detect_vgg_golden.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
