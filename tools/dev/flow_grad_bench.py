"""Times the three backward entry points (ft_correlation_bwd, ft_resample2d_bwd, ft_channelnorm_bwd) at FlowNet2 shapes.

    python tools/dev/flow_grad_bench.py [--iters 50] [--warmup 10] [--out profiles/flow_grad_bench.json]

Each call is timed alone with device events after a warm-up; the JSON gives the median and minimum per call, the target of
the issue, and the floor from the bounding roof (fp32 peak for Correlation, HBM bandwidth for the other two).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from flowtrack.pytorch_amd import _lib, synth  # noqa: E402
from flowtrack.pytorch_amd._lib import check  # noqa: E402

FP32_PEAK = 157.3e12      # FLOP/s, vector = matrix on gfx950
HBM = 6.3e12              # B/s, achievable streaming rate used for the floors


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []

    # Correlation, FlowNetC parameters (FlowNetC.py:28,31) at the configs[3] map: [16, 256, 48, 64]
    B, C, H, W = 16, 256, 48, 64
    pad, k, md, s1, s2 = 20, 1, 20, 1, 2
    a = synth.normal(1, "a", (B, C, H, W)).to(dev)
    b = synth.normal(1, "b", (B, C, H, W)).to(dev)
    g = synth.normal(1, "g", (B, 441, H, W)).to(dev)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    flops = 2 * 2.0 * B * C * H * W * 441
    for name, p1, p2 in (("correlation_bwd both", ga, gb), ("correlation_bwd grad_in1", ga, None), ("correlation_bwd grad_in2", None, gb)):
        def fn(p1=p1, p2=p2):
            check(lib.ft_correlation_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), p1.data_ptr() if p1 is not None else None,
                                         p2.data_ptr() if p2 is not None else None, B, C, H, W, pad, k, md, s1, s2, 1, s))
        med, mn = _time(fn, args.iters, args.warmup)
        f = flops if p1 is not None and p2 is not None else flops / 2
        rows.append({"op": name, "shape": [B, C, H, W], "median_us": round(med, 1), "min_us": round(mn, 1),
                     "target_us": 350.0 if p1 is not None and p2 is not None else None, "gflop": round(f / 1e9, 2),
                     "floor_us": round(f / FP32_PEAK * 1e6, 1), "roof": "fp32 157.3 TF",
                     "share_of_roof": round(f / FP32_PEAK * 1e6 / med, 3)})
    del a, b, g, ga, gb

    # Resample2d at the configs[3] image: [16, 3, 384, 512], smooth (synth.flow_field) and per-pixel N(0, 4 px) flows
    B, C, H, W = 16, 3, 384, 512
    img = synth.normal(2, "img", (B, C, H, W)).to(dev)
    go = synth.normal(2, "go", (B, C, H, W)).to(dev)
    gi, gf = torch.empty_like(img), torch.empty((B, 2, H, W), device=dev)
    nbytes = 4.0 * B * H * W * (3 * C + 2 * 2)
    for kind, target in (("smooth", 60.0), ("noise", 90.0)):
        flow = (synth.flow_field(2, B, H, W, magnitude=6.0) if kind == "smooth" else synth.normal(2, "nf", (B, 2, H, W)) * 4.0).to(dev)
        for part, p1, p2 in (("both", gi, gf), ("grad_in1", gi, None), ("grad_flow", None, gf)):
            def fn(p1=p1, p2=p2, flow=flow):
                check(lib.ft_resample2d_bwd(img.data_ptr(), flow.data_ptr(), go.data_ptr(), p1.data_ptr() if p1 is not None else None,
                                            p2.data_ptr() if p2 is not None else None, B, C, H, W, s))
            med, mn = _time(fn, args.iters, args.warmup)
            row = {"op": f"resample2d_bwd {part} ({kind} flow)", "shape": [B, C, H, W], "median_us": round(med, 1),
                   "min_us": round(mn, 1), "target_us": target if part == "both" else None}
            if part == "both":
                row.update({"mbytes": round(nbytes / 1e6, 1), "floor_us": round(nbytes / HBM * 1e6, 1), "roof": "HBM 6.3 TB/s",
                            "share_of_roof": round(nbytes / HBM * 1e6 / med, 3)})
            rows.append(row)

    # ChannelNorm at the same image
    x = synth.normal(3, "x", (B, C, H, W)).to(dev)
    out = torch.sqrt((x * x).sum(1, keepdim=True))
    gn = synth.normal(3, "gn", (B, 1, H, W)).to(dev)
    gx = torch.empty_like(x)

    def fn():
        check(lib.ft_channelnorm_bwd(x.data_ptr(), out.data_ptr(), gn.data_ptr(), gx.data_ptr(), B, C, H, W, s))
    med, mn = _time(fn, args.iters, args.warmup)
    nbytes = 4.0 * B * H * W * (2 * C + 2)
    rows.append({"op": "channelnorm_bwd", "shape": [B, C, H, W], "median_us": round(med, 1), "min_us": round(mn, 1), "target_us": 25.0,
                 "mbytes": round(nbytes / 1e6, 1), "floor_us": round(nbytes / HBM * 1e6, 1), "roof": "HBM 6.3 TB/s",
                 "share_of_roof": round(nbytes / HBM * 1e6 / med, 3)})

    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rows": rows}
    for r in rows:
        print(f"{r['op']:<44s} {r['median_us']:9.1f} us (min {r['min_us']:.1f})" +
              (f"  target {r['target_us']:.0f}" if r.get("target_us") else "") +
              (f"  floor {r['floor_us']:.1f} ({r['roof']})" if r.get("floor_us") else ""))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
