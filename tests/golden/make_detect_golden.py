#!/usr/bin/env python3
"""Generates tests/golden/detect_golden.npz by importing and running the ORIGINAL reference's detector glue on CPU:
lib/detection/model/bbox_transform.py, layer_utils/snippets.py (+ generate_anchors.py) and layer_utils/proposal_layer.py.  Like
make_golden.py it needs the reference checkout, so nothing in tests/, bench.py or smoke() ever runs this file; they only read the
.npz it wrote.  Two of the reference's imports cannot be met here and are replaced before it is imported: `easydict` (not
installed; a dict with attribute access stands in) and `model.nms_wrapper` (it binds the CUDA-only nms `_ext`; the restated
IoU > thresh NMS of tests/detect_ref.py is injected, which is what the reference's detector runs on the GPU).

Stored (data only, tens of kilobytes):
  anchors_5x7, anchors_3x4, count_5x7, count_3x4   generate_anchors_pre at stride 16, default scales / ratios
  dec_deltas, dec_im, dec_boxes                    bbox_transform_inv + clip_boxes of the 315 anchors of the 5x7 map, |d| <= 1
  prop_cls_prob, prop_bbox_pred, prop_im_info, prop_pre, prop_post, prop_thresh, prop_blob, prop_scores
                                                   one proposal_layer case on the 5x7 map (pre 200, post 30, 0.7)
  seed

The seed is the first from SEED0 upwards at which the proposal case's OWN inputs satisfy, on the CPU and from the reference alone:
all scores distinct, and no pair of the pre-NMS boxes has a float64 IoU within 1e-4 of the threshold — far above what the decode
error bound (tests/detect_ref.py: decode_bound, < 1e-3 px) can move an IoU for boxes of tens to hundreds of pixels — so the kept
set cannot depend on expf ulps.  The file is written with fixed zip timestamps: it regenerates byte-equal.
"""
from __future__ import annotations

import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref  # noqa: E402

SEED0 = 20261019
IOU_GUARD = 1e-4
PRE, POST, THRESH = 200, 30, 0.7
NUM_ANCHORS = 9


class _AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def import_reference_detection():
    easydict = types.ModuleType("easydict")
    easydict.EasyDict = _AttrDict
    sys.modules["easydict"] = easydict
    sys.path.insert(0, os.path.join(REF, "lib", "detection"))
    import model  # noqa: F401  (the reference's package)
    wrapper = types.ModuleType("model.nms_wrapper")

    def nms(dets, thresh):
        return torch.from_numpy(detect_ref.nms(dets.numpy(), thresh, inclusive=False).astype(np.int64))

    wrapper.nms = nms
    sys.modules["model.nms_wrapper"] = wrapper
    from layer_utils import proposal_layer as pl, snippets
    from model import bbox_transform
    from model.config import cfg
    return snippets, bbox_transform, pl, cfg


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def inputs(seed, count):
    rng = np.random.RandomState(seed % (2 ** 32))
    deltas = rng.uniform(-1.0, 1.0, (count, 4)).astype(np.float32)
    deltas[:, :2] *= np.float32(0.5)
    cls_prob = rng.uniform(0.0, 1.0, (1, 5, 7, 2 * NUM_ANCHORS)).astype(np.float32)
    return deltas, cls_prob


def main():
    snippets, bbox_transform, pl, cfg = import_reference_detection()
    out = {}
    for h, w in ((5, 7), (3, 4)):
        anchors, count = snippets.generate_anchors_pre(h, w, 16)
        out[f"anchors_{h}x{w}"], out[f"count_{h}x{w}"] = anchors, np.int32(count)
    anchors = out["anchors_5x7"]
    im_info = np.array([300.0, 400.0, 1.0], dtype=np.float32)
    cfg.TEST.RPN_PRE_NMS_TOP_N, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.TEST.RPN_NMS_THRESH = PRE, POST, THRESH
    seed = SEED0
    while True:
        deltas, cls_prob = inputs(seed, len(anchors))
        with torch.no_grad():
            boxes = bbox_transform.clip_boxes(bbox_transform.bbox_transform_inv(torch.from_numpy(anchors), torch.from_numpy(deltas)),
                                              im_info[:2]).numpy()
        scores = cls_prob[:, :, :, NUM_ANCHORS:].reshape(-1)
        top = np.argsort(-scores, kind="stable")[:PRE]
        iou = detect_ref.iou_matrix(boxes[top], np.float64)
        distinct = len(np.unique(scores)) == len(scores)
        guard = np.abs(iou[np.triu_indices(len(top), 1)] - THRESH).min()
        if distinct and guard > IOU_GUARD:
            break
        seed += 1
    assert distinct, "the proposal case's scores must be distinct"
    assert guard > IOU_GUARD, f"a pre-NMS pair has an IoU within {IOU_GUARD} of {THRESH}"
    bbox_pred = deltas.reshape(1, 5, 7, 4 * NUM_ANCHORS)
    with torch.no_grad():
        blob, kept_scores = pl.proposal_layer(torch.from_numpy(cls_prob), torch.from_numpy(bbox_pred), im_info, "TEST", 16,
                                              torch.from_numpy(anchors), NUM_ANCHORS)
    out.update(dec_deltas=deltas, dec_im=im_info[:2], dec_boxes=boxes, prop_cls_prob=cls_prob, prop_bbox_pred=bbox_pred,
               prop_im_info=im_info, prop_pre=np.int32(PRE), prop_post=np.int32(POST), prop_thresh=np.float32(THRESH),
               prop_blob=blob.numpy(), prop_scores=kept_scores.numpy(), seed=np.int64(seed))
    path = os.path.join(HERE, "detect_golden.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes; seed", seed, "; kept", len(blob), "; min |IoU - thresh|", guard)


if __name__ == "__main__":
    main()
