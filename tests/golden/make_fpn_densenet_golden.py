#!/usr/bin/env python3
"""Generates tests/golden/fpn_densenet_golden.npz by importing and running the ORIGINAL reference's models.fpn('densenet121') on
CPU (the recipe of make_fpn_golden.py).  It needs the reference checkout, so nothing in tests/, bench.py or smoke() ever runs this
file; they only read the .npz it wrote.

Weights and inputs are not stored: both sides regenerate them from flowtrack.pytorch_amd.synth (fill_densenet_state_dict on the
reference's own state_dict, pose_crops).  Stored, per shape (B=2 128x96: c5 = 4x3, heat maps 32x24; B=3 64x64: c5 = 2x2, the smallest
legal map): the reference's heat maps, max_preds indices and scores, the top-1 / top-2 margin of every map; once: the seed, the
largest magnitude of any dense-block output, and the reference's state_dict keys with their shapes.

The seed is the first from SEED0 upwards at which, in the reference's own run at both shapes,
  * max |heat map| <= 16 (one fp32 ulp at 16 is 1e-6: room for a deep net under the absolute 1e-3 bound of the fp32 tests),
  * max |any dense-block output| <= 1024 (fp16 headroom),
  * every map with score > 0 has a top-1 / top-2 margin >= 4e-3 (twice the gap a per-element error of 1e-3 can close),
  * tests/fpn_densenet_ref.py::fpn_densenet_forward reproduces the imported reference to 1e-5;
the script aborts if no seed in range does.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(make_golden.ROOT, "tests"))
import fpn_densenet_ref  # noqa: E402
from flowtrack.pytorch_amd import synth  # noqa: E402
from oracle import keypoints_ref  # noqa: E402

SEED0 = 20261021
SHAPES = ((2, 128, 96), (3, 64, 64))
MIN_MARGIN = 4e-3
MAX_HEAT = 16.0
MAX_BLOCK = 1024.0


def run_seed(net, ref_eval, seed):
    sd = synth.fill_densenet_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    out, ok, block_max = {}, True, 0.0
    for B, H, W in SHAPES:
        x = synth.pose_crops(seed, B, H, W)
        with torch.no_grad():
            hm_ref = net(x)
        mine, feats = fpn_densenet_ref.fpn_densenet_forward(sd, x, depth=121, return_features=True)
        err = (hm_ref - mine).abs().max().item()
        assert err <= 1e-5, f"tests/fpn_densenet_ref.py::fpn_densenet_forward does not reproduce the imported reference ({err:.3e})"
        bmax = max(float(feats[f"layer{i}"].abs().max()) for i in (1, 2, 3, 4))
        block_max = max(block_max, bmax)
        hm = hm_ref.numpy()
        r_coords, r_scores = ref_eval.max_preds(hm_ref)
        o_coords, o_scores, o_idx = keypoints_ref.max_preds_ref(hm)
        assert np.array_equal(r_scores, o_scores) and np.array_equal(r_coords[..., 0], o_coords[..., 0])
        margin = make_golden.top2_margin(hm)
        live = o_scores[..., 0] > 0
        worst = float(margin[live].min()) if live.any() else float("inf")
        print(f"seed {seed} {B}x{H}x{W}: range [{hm.min():.3f}, {hm.max():.3f}], dense-block outputs up to {bmax:.1f}, restatement vs reference "
              f"{err:.2e}, {int(live.sum())}/{live.size} maps with score > 0, smallest margin among them {worst:.3e}")
        ok = ok and worst >= MIN_MARGIN and float(np.abs(hm).max()) <= MAX_HEAT and bmax <= MAX_BLOCK
        tag = f"b{B}_{H}x{W}"
        out[tag + "_heatmaps"] = hm.astype(np.float32)
        out[tag + "_idx"] = o_idx.astype(np.int32)
        out[tag + "_scores"] = o_scores.astype(np.float32)
        out[tag + "_margin"] = margin
    out["block_max"] = np.array(block_max, dtype=np.float32)
    return out, ok


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_pose, ref_eval = make_golden.import_reference_pose()
    net = ref_pose.fpn("densenet121", num_classes=17, pretrained=False).eval()
    assert net.planes == fpn_densenet_ref.planes(121)
    keys = [(k, tuple(v.shape), str(v.dtype)) for k, v in net.state_dict().items()]
    for seed in range(SEED0, SEED0 + 32):
        out, ok = run_seed(net, ref_eval, seed)
        if ok:
            break
    else:
        raise SystemExit("no seed in range meets the fixture's conditions")
    for B, H, W in SHAPES:      # the assertions the fixture is committed under
        tag = f"b{B}_{H}x{W}"
        live = out[tag + "_scores"][..., 0] > 0
        assert (out[tag + "_margin"][live] >= MIN_MARGIN).all() and np.abs(out[tag + "_heatmaps"]).max() <= MAX_HEAT
    assert out["block_max"] <= MAX_BLOCK
    out["seed"] = np.array(seed)
    out["shapes"] = np.array(SHAPES)
    out["min_margin"] = np.array(MIN_MARGIN)
    out["state_dict_keys"] = np.array(["%s %s %s" % (k, "x".join(str(d) for d in s), d) for k, s, d in keys])
    path = os.path.join(HERE, "fpn_densenet_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
