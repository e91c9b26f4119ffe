"""The VGG16 detector's new launches alone (dev tool): python tools/dev/vgg_bench.py [rows=300] [H=600 W=1000]

  * classifier.0 (25088 -> 4096) and classifier.3 (4096 -> 4096) + ReLU at `rows` RoI rows, fp16, in both recorded forms: "fc" =
    ft_fc_fwd, "igemm" = ft_conv2d_fwd on the [rows,1,1,K] view (with its own first-call tile / direct-form benchmark).  Each form
    is one captured plan, replayed back to back; the two forms alternate over five windows and the median window is reported, next
    to the time 6.3 TB/s needs for the weights alone.  Back-to-back replays find the 34 MB of classifier.3 in the memory-side
    cache; the in-situ figure is the region-head table of `net_bench.py frcnn_vgg16`.
  * the four ft_maxpool2x2s2_fwd launches of an H x W blob, fp16, next to 6.3 TB/s over the bytes they move.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.engine import HipModule
from flowtrack.pytorch_amd.hip_ops import ActView, FusedConv, FusedFC, Program, new_act, record_maxpool2x2

HBM = 6.3e12
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 300
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (600, 1000)
dev = torch.device("cuda")
host = HipModule()
stream = torch.cuda.Stream()


def window(prog, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cur = torch.cuda.current_stream()
    for _ in range(3):
        prog.run(cur)
    a.record()
    for _ in range(iters):
        prog.run(cur)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3            # us


def plan_of(record):
    prog = Program(stream)
    record(prog)
    host._run_plan(prog, first=True)                  # eager run, tile / choice benchmark, capture
    torch.cuda.synchronize()
    return prog


for name, k, n in (("classifier.0", 25088, 4096), ("classifier.3", 4096, 4096)):
    w = synth.uniform(1, name, (n, k), -0.02, 0.02)
    bias = synth.normal(1, name + ".b", (n,), std=0.05)
    x = new_act(rows, 1, 1, k, torch.float16, dev)
    x.t.copy_(synth.normal(1, name + ".x", (rows, 1, 1, k)).half())
    ys = {f: new_act(rows, 1, 1, n, torch.float16, dev) for f in ("fc", "igemm")}
    fc = FusedFC(w, bias, device=dev, act="relu", label=name)
    conv = FusedConv(w[:, :, None, None], dtype=torch.float16, device=dev, bias=bias, act="relu", label=name)
    progs = {"fc": plan_of(lambda p: fc.record(p, x, ys["fc"])), "igemm": plan_of(lambda p: conv.record(p, x, ys["igemm"]))}
    diff = float((ys["fc"].t.float() - ys["igemm"].t.float()).abs().max())
    times = {f: [] for f in progs}
    for _ in range(5):
        for f, prog in progs.items():
            times[f].append(window(prog, 50))
    floor = n * k * 2 / HBM * 1e6
    kept = [c[0] for c in progs["igemm"].calls]
    print(f"{name} {rows} x {k} -> {n} fp16: " + ", ".join(f"{f} {np.median(t):8.1f} us (windows {min(t):.1f} - {max(t):.1f})" for f, t in times.items())
          + f"; weights at 6.3 TB/s {floor:.1f} us; igemm plan kept {kept}; max |fc - igemm| {diff:.2e}; "
          + f"{2.0 * rows * k * n / np.median(times['fc']) * 1e-6:.0f} / {2.0 * rows * k * n / np.median(times['igemm']) * 1e-6:.0f} TFLOP/s")
    del fc, conv, progs, w

cur_h, cur_w = H, W
for c in (64, 128, 256, 512):
    x = new_act(1, cur_h, cur_w, c, torch.float16, dev)
    x.t.copy_(torch.randn(x.t.shape, device=dev).half())
    y = new_act(1, cur_h // 2, cur_w // 2, c, torch.float16, dev)
    prog = plan_of(lambda p: record_maxpool2x2(p, x, y))
    t = [window(prog, 100) for _ in range(5)]
    moved = (x.t.numel() + y.t.numel()) * 2
    print(f"ft_maxpool2x2s2_fwd [1,{cur_h},{cur_w},{c}] fp16: {np.median(t):7.1f} us (windows {min(t):.1f} - {max(t):.1f}); {moved / 1e6:.1f} MB moved, "
          f"{moved / HBM * 1e6:.1f} us at 6.3 TB/s; {moved / np.median(t) * 1e-6:.2f} TB/s")
    cur_h, cur_w = cur_h // 2, cur_w // 2
