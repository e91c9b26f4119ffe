"""Times ft_bottleneck_fwd alone (layer1 block at batch B): usage bnk_bench.py [B] [H] [W] [exit[:full|even|none]]; FT_BNK_DBG knobs apply.
With `exit` the launch timed is ft_bottleneck_exit_fwd (the block + layer2.0.conv1, y mode `even` unless given) and, for comparison,
the pair of launches it replaces (ft_bottleneck_fwd, then the 256 -> 128 conv on its output)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.hip_ops import ActView, FusedConv, Program, record_bottleneck, record_bottleneck_exit
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
H = int(sys.argv[2]) if len(sys.argv) > 2 else 64
W = int(sys.argv[3]) if len(sys.argv) > 3 else 48
dev, dt = torch.device("cuda:0"), torch.float16
bn = lambda c: {"weight": torch.ones(c), "bias": torch.zeros(c), "running_mean": torch.zeros(c), "running_var": torch.ones(c), "eps": 1e-5}
mk = dict(dtype=dt, device=dev, act="relu")
c1 = FusedConv(synth.normal(1, "w1", (64, 256, 1, 1), std=0.08), bn=bn(64), **mk)
c2 = FusedConv(synth.normal(1, "w2", (64, 64, 3, 3), std=0.06), pad=1, bn=bn(64), **mk)
c3 = FusedConv(synth.normal(1, "w3", (256, 64, 1, 1), std=0.17), bn=bn(256), **mk)
x = ActView(torch.randn((B, H, W, 256), device=dev).to(dt), 256, 0)
y = ActView(torch.zeros((B, H, W, 256), dtype=dt, device=dev), 256, 0)
y2 = ActView(torch.zeros((B, H, W, 256), dtype=dt, device=dev), 256, 0)
if len(sys.argv) > 4 and sys.argv[4].startswith("exit"):
    mode = sys.argv[4].partition(":")[2] or "even"
    tail = FusedConv(synth.normal(1, "wt", (128, 256, 1, 1), std=0.08), bn=bn(128), **mk)
    t1 = ActView(torch.zeros((B, H, W, 128), dtype=dt, device=dev), 128, 0)
    ye = None if mode == "none" else (y if mode == "full" else ActView(torch.zeros((B, H // 2, W // 2, 256), dtype=dt, device=dev), 256, 0))
    prog = Program(torch.cuda.Stream())
    for _ in range(4):       # the exit launch, then the two launches it replaces, on the same input
        record_bottleneck_exit(prog, c1, c2, c3, tail, x, ye, t1, "exit", mode)
        record_bottleneck(prog, c1, c2, c3, x, y2, "block", form="patch")
        tail.record(prog, y2, t1)
    prog.resolve_choices()
    torch.cuda.synchronize()
    prog.run_eager(); prog.stream.synchronize()
    t = prog.time_calls(iters=10, median=True)
    us = {}
    for name, ms in t:
        us.setdefault(name, []).append(ms * 1e3)
    avg = {k: sum(v) / len(v) for k, v in us.items()}
    pair = sum(v for k, v in avg.items() if k != "ft_bottleneck_exit_fwd")
    print(f"FT_BNK_DBG={os.environ.get('FT_BNK_DBG', '0'):>3s}  B={B} {H}x{W} y={mode}: exit form {avg['ft_bottleneck_exit_fwd']:7.1f} us   the two launches {pair:7.1f} us  ("
          + ", ".join(f"{k} {v:.1f}" for k, v in avg.items() if k != "ft_bottleneck_exit_fwd") + ")", flush=True)
    sys.exit(0)
prog = Program(torch.cuda.Stream())
for _ in range(4):           # ping-pong like the network does, 4 launches per pass
    record_bottleneck(prog, c1, c2, c3, x, y, "a", form="patch")      # the kernel the FT_BNK_DBG knobs belong to, as the network records it
    record_bottleneck(prog, c1, c2, c3, y, y2, "b", form="patch")
torch.cuda.synchronize()
prog.run_eager(); prog.stream.synchronize()
t = prog.time_calls(iters=10)
us = sum(ms for _, ms in t) / len(t) * 1e3
gb = 2 * B * H * W * 256 * 2 / 1e9
print(f"FT_BNK_DBG={os.environ.get('FT_BNK_DBG', '0'):>3s}  B={B} {H}x{W}: {us:7.1f} us per block   {gb / us * 1e3:6.2f} TB/s algorithmic", flush=True)
