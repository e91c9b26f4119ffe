#!/usr/bin/env python3
"""Generates tests/golden/hg_golden.npz by importing and running the ORIGINAL reference's models.hg on CPU (the recipe of
make_golden.py::import_reference_pose).  It needs the reference checkout, so nothing in tests/, bench.py or smoke() ever runs this
file; they only read the .npz it wrote.

Weights and inputs are not stored: both sides regenerate them from flowtrack.pytorch_amd.synth (fill_hg_state_dict on the
reference's own state_dict, pose_crops).  Configurations: num_stacks = 8 (one block per chain) at B=2 64x64 (the smallest legal
input: the lowest level is 1x1) and B=2 96x80 (maps of 24x20, 12x10, 6x5, 3x2, 1x1: odd sizes on the way down), num_stacks = 2
(chains of four blocks) at B=2 96x80.  Stored per configuration: every stack's heat maps, the last stack's max_preds indices and
scores, the top-1 / top-2 margin of every map of every stack, the largest activation of the reference's forward; per num_stacks the
reference's state_dict keys with their shapes; once the seed.

Conditions the fixture is committed under (asserted below):
  * tests/hourglass_ref.py::hg_forward reproduces the imported reference to 1e-5 of each map's range;
  * the reference's largest activation is <= 4096 at every configuration (16x headroom in fp16);
  * at least 3/4 of the last stack's maps with score > 0 have a margin >= 2 tol, tol = hourglass_ref.stack_tol(range of the last
    stack's maps): the seed is the first from SEED0 upwards that gives this at every configuration.  (The hourglass's maps are
    smooth: near-ties between neighbouring pixels are a property of the maps, and the tests account for each one by its margin.)
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
import hourglass_ref  # noqa: E402
from flowtrack.pytorch_amd import synth  # noqa: E402
from oracle import keypoints_ref  # noqa: E402

SEED0 = 20261019
CONFIGS = ((8, 2, 64, 64), (8, 2, 96, 80), (2, 2, 96, 80))          # (num_stacks, B, H, W)
MAX_PEAK = 4096.0
MIN_LIVE_FRACTION = 0.75


def tag_of(cfg):
    return "s%d_b%d_%dx%d" % cfg


def reference_peak(net, x):
    """The reference's forward with a hook on every leaf module: (list of heat maps, largest |output| of any module)."""
    peak = [0.0]

    def hook(_m, _i, o):
        peak[0] = max(peak[0], float(o.abs().max()))
    handles = [m.register_forward_hook(hook) for m in net.modules() if not list(m.children())]
    with torch.no_grad():
        out = net(x)
    for h in handles:
        h.remove()
    return out, peak[0]


def run_seed(nets, ref_eval, seed):
    out, ok = {}, True
    for cfg in CONFIGS:
        S, B, H, W = cfg
        net = nets[S]
        sd = synth.fill_hg_state_dict(net.state_dict(), seed)
        net.load_state_dict(sd)
        x = synth.pose_crops(seed, B, H, W)
        hm_ref, peak = reference_peak(net, x)
        mine, my_peak = hourglass_ref.hg_forward(sd, x, S, return_peak=True)
        assert len(hm_ref) == len(mine) == S
        peak = max(peak, my_peak)         # (hg_forward also sees the sums: the hooks see module outputs only)
        for i, (a, b) in enumerate(zip(hm_ref, mine)):
            rng = float(a.max() - a.min())
            err = float((a - b).abs().max())
            assert err <= 1e-5 * rng, f"hourglass_ref.hg_forward does not reproduce the imported reference (stack {i}: {err:.3e} on {rng:.3e})"
        assert peak <= MAX_PEAK, f"largest activation {peak:.3e} > {MAX_PEAK}"
        hms = np.stack([t.numpy() for t in hm_ref]).astype(np.float32)          # [S, B, K, h, w]
        last = hms[-1]
        r_coords, r_scores = ref_eval.max_preds(hm_ref[-1])
        o_coords, o_scores, o_idx = keypoints_ref.max_preds_ref(last)
        assert np.array_equal(r_scores, o_scores) and np.array_equal(r_coords[..., 0], o_coords[..., 0])
        margin = np.stack([make_golden.top2_margin(h) for h in hms])            # [S, B, K]
        tol = hourglass_ref.stack_tol(last.max() - last.min())
        live = o_scores[..., 0] > 0
        good = int((margin[-1][live] >= 2 * tol).sum())
        print(f"seed {seed} {tag_of(cfg)}: last-stack range [{last.min():.3f}, {last.max():.3f}] tol {tol:.3e}, peak activation {peak:.3e}, "
              f"{int(live.sum())}/{live.size} live maps, {good} of them with margin >= 2 tol")
        ok = ok and live.sum() > 0 and good >= MIN_LIVE_FRACTION * live.sum()
        t = tag_of(cfg)
        out[t + "_heatmaps"] = hms
        out[t + "_idx"] = o_idx.astype(np.int32)
        out[t + "_scores"] = o_scores.astype(np.float32)
        out[t + "_margin"] = margin.astype(np.float32)
        out[t + "_peak"] = np.array(peak, dtype=np.float32)
    return out, ok


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_pose, ref_eval = make_golden.import_reference_pose()
    nets = {S: ref_pose.hg(num_classes=17, num_stacks=S).eval() for S in sorted({c[0] for c in CONFIGS})}
    for seed in range(SEED0, SEED0 + 16):
        out, ok = run_seed(nets, ref_eval, seed)
        if ok:
            break
    else:
        raise SystemExit("no seed in range gives 3/4 of the live maps a margin >= 2 tol at every configuration")
    for cfg in CONFIGS:      # the assertions the fixture is committed under
        t = tag_of(cfg)
        last = out[t + "_heatmaps"][-1]
        live = out[t + "_scores"][..., 0] > 0
        tol = hourglass_ref.stack_tol(last.max() - last.min())
        assert (out[t + "_margin"][-1][live] >= 2 * tol).sum() >= MIN_LIVE_FRACTION * live.sum() > 0
        assert out[t + "_peak"] <= MAX_PEAK
    out["seed"] = np.array(seed)
    out["configs"] = np.array(CONFIGS)
    for S, net in nets.items():
        out[f"state_dict_keys_s{S}"] = np.array(["%s %s %s" % (k, "x".join(str(d) for d in v.shape), v.dtype) for k, v in net.state_dict().items()])
    path = os.path.join(HERE, "hg_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
