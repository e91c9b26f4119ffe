"""The whole flip-test step, two forms, alternated in one process (dev tool):  python tools/dev/flip_bench.py [--steps 50] [--rounds 4]

R50, fp16, 64 crops of 256x192 (synthetic), key-point rows on the device as the result of a step:
  (a) two-pass eager  the generic path of tools/pose/main.validate, restated: model(x), model(torch.flip(x)), torch.flip + channel
                      index of the second heat maps, add, multiply, then max_preds (+ nudge) of the average — two 64-crop plan
                      replays and the eager glue between and behind them;
  (b) flip plan       DeconvResnet.flip_pairs + keypoints_in_plan: ONE graph replay (ft_hflip_nchw_f32, the trunk and head at 128
                      crops, ft_heatmap_flip_merge writing the rows).
Both take the same device tensor x (each stages it into its plan's input).  Device events around windows of --steps steps, both forms
warmed first, windows alternated a, b, a, b, ...; prints every window, the medians, the spread and the ratio, and a JSON line.  The two
forms' rows are compared once before timing (the score column within the fp16 bar, as the two forms run different plans)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flowtrack.pytorch_amd import synth  # noqa: E402
from flowtrack.pytorch_amd.pose import evaluation, models  # noqa: E402
from tools.pose.main import COCO_FLIP_PAIRS, _flip_back  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="steps per timed window (>= 50)")
    ap.add_argument("--rounds", type=int, default=4, help="alternations a, b (>= 3)")
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args(argv)
    if args.steps < 50 or args.rounds < 3:
        raise SystemExit("at least 50 steps per window and three alternations")
    B, H, W = args.batch, 256, 192
    m = models.deconv("resnet50", 17, False)
    m.load_state_dict(synth.fill_pose_state_dict(m.state_dict(), 1))
    m = m.cuda().eval()
    m.compute_dtype = torch.float16
    x = synth.pose_crops(1, B, H, W).cuda()

    def two_pass():
        m.flip_pairs, m.keypoints_in_plan = None, None
        out = m(x)
        flipped = _flip_back(m(torch.flip(x, dims=[3])), COCO_FLIP_PAIRS)
        out = (out + flipped) * 0.5
        _, score, coords = evaluation.heatmap_max_preds(out, adjust_coords=True)
        return torch.cat((coords, score), dim=2)

    def flip_plan():
        m.flip_pairs, m.keypoints_in_plan = COCO_FLIP_PAIRS, True
        return m.forward_keypoint_rows(x)

    forms = (("two_pass_eager", two_pass), ("flip_plan", flip_plan))
    for _ in range(5):                                     # warm-up of both forms: plans, tile picks, graphs, torch's own kernels
        rows = [fn().clone() for _, fn in forms]
    torch.cuda.synchronize()
    same_xy = (rows[0][..., :2] == rows[1][..., :2]).all(dim=2).float().mean().item()
    print(f"rows: {same_xy:.4f} of the key points identical between the forms, largest score difference "
          f"{(rows[0][..., 2] - rows[1][..., 2]).abs().max().item():.3e} (different plans: split-K tile picks differ)")
    ms = {name: [] for name, _ in forms}
    for r in range(args.rounds):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
            print(f"round {r} {name:15s} {ms[name][-1]:8.4f} ms/step")
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k:15s} median {med[k]:.4f} ms/step (min {min(v):.4f}, max {max(v):.4f}; {B / med[k] * 1e3:.0f} crops/s)")
    ratio = med["two_pass_eager"] / med["flip_plan"]
    print(f"two-pass eager / flip plan = {ratio:.3f}")
    print(json.dumps({"batch": B, "res": [H, W], "steps": args.steps, "rounds": args.rounds, "ms_per_step": ms, "median_ms": med, "ratio": ratio}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
