"""Times the detector's region-stage entry points (csrc/detect_ops.hip) at the detector's own shapes.

    python tools/dev/detect_bench.py [--iters 30] [--warmup 5] [--out detect_bench.json]
    python tools/dev/detect_bench.py --clip [--frames 32] [--rounds 5] [--nets res101,vgg16] [--out detect_clip_bench.json]

Shapes: a 600 x 1000 image at stride 16 -> features [1,1024,38,63], 9 anchors per cell = 21 546 boxes to decode, NMS over the top
6000 of them, 300 RoIs.  Each call is timed alone with device events after a warm-up; printed per entry: the median and minimum
in microseconds, the bytes it has to move (every input and output element once, the NMS mask written and read once) and the
ratio of that floor at the achievable HBM rate to the measured median.

--clip: the detector over a clip, two forms alternated in one process (windows a, b, a, b, ... as tools/dev/flip_bench.py), fp16, 81
classes, synthetic weights, T frames of 600 x 1000 (blob scale 1) resident on the device:
  (a) per frame   a loop of detection.test.detect_persons: per frame two torch.sort calls, two count reads, one download;
  (b) clip        detection.test.detect_persons_clip: every frame step enqueued without a host wait, one download.
A window is one pass over the T frames, host-timed between device synchronisations (form (a) is bound by the host, which device
events around it would also see, but only as a whole).  Both forms are warmed first and their results compared bit for bit.  Also
event-times ft_topk_desc_f32 at n = 21 546, k = 6000 against the torch.sort + slice it replaces, on spread scores and on scores
within two ulps of 0.5 (what synthetic RPN heads give).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flowtrack.pytorch_amd import _lib  # noqa: E402
from flowtrack.pytorch_amd._lib import FT_F16, FT_F32, check  # noqa: E402
from flowtrack.pytorch_amd.detection import proposal  # noqa: E402

HBM = 6.3e12              # B/s, achievable streaming rate used for the floors
B, C, H, W, R, POOLED = 1, 1024, 38, 63, 300, 7
IM_H, IM_W = 600.0, 1000.0
N_NMS = 6000


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


def clip_main(args):
    import statistics
    import time

    from flowtrack.pytorch_amd import synth
    from flowtrack.pytorch_amd.detection import nets, test as det_test
    dev = torch.device("cuda:0")
    T, K, person = args.frames, 81, 1
    frames = torch.from_numpy(np.stack([synth.detector_frame(t, 600, 1000) for t in range(T)])).to(dev)
    report = {"frames": T, "rounds": args.rounds, "nets": {}}
    for name in args.nets.split(","):
        net = nets.vgg16() if name == "vgg16" else nets.resnetv1(int(name[3:]))
        net.create_architecture(K, tag="default")
        fill = synth.fill_vgg_detector_state_dict if name == "vgg16" else synth.fill_detector_state_dict
        net.load_state_dict(fill(net.state_dict(), 1))
        net = net.to(dev).eval()
        net.compute_dtype = torch.float16

        def per_frame():
            return [det_test.detect_persons(net, frames[t], person, 0.3) for t in range(T)]

        def clip():
            return det_test.detect_persons_clip(net, frames, person, 0.3)

        forms = (("per_frame", per_frame), ("clip", clip))
        for _ in range(2):                                  # plans, tile picks, graphs, torch's own kernels
            outs = [fn() for _, fn in forms]
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*outs))
        print(f"{name}: {T} frames, {sum(len(d) for d in outs[0])} person boxes, clip == per frame bit for bit: {same}")
        ms = {k: [] for k, _ in forms}
        for r in range(args.rounds):
            for k, fn in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / T)
                print(f"{name} round {r} {k:10s} {ms[k][-1]:8.4f} ms/frame")
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            print(f"{name} {k:10s} median {med[k]:.4f} ms/frame (min {min(v):.4f}, max {max(v):.4f}; {1e3 / med[k]:.0f} frames/s)")
        print(f"{name} per frame / clip = {med['per_frame'] / med['clip']:.3f}")
        report["nets"][name] = {"ms_per_frame": ms, "median_ms": med, "ratio": med["per_frame"] / med["clip"], "bit_equal": bool(same)}
        del net
    # the sort alone
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n, k = 21546, N_NMS
    rng = np.random.RandomState(0)
    inputs = {"spread": rng.permutation(n).astype(np.float32) / n,
              "near_half": (np.uint32(0x3F000000) + rng.randint(-2, 3, n)).astype(np.uint32).view(np.float32)}
    order, out = torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.float32, device=dev)
    report["topk"] = {}
    for label, host in inputs.items():
        sc = torch.from_numpy(host).to(dev)

        def torch_sort():
            v, i = sc.sort(descending=True, stable=True)
            return v[:k], i[:k]

        check(lib.ft_topk_desc_f32(p(sc), n, k, p(order), p(out), None, stream), "ft_topk_desc_f32")
        tv, ti = torch_sort()
        ok = bool(torch.equal(ti, order.long()) and torch.equal(tv.view(torch.int32), out.view(torch.int32)))
        a = _time(lambda: lib.ft_topk_desc_f32(p(sc), n, k, p(order), p(out), None, stream), args.iters, args.warmup)
        b = _time(torch_sort, args.iters, args.warmup)
        print(f"top {k} of {n} ({label}): ft_topk_desc_f32 median {a[0]:.2f} us (min {a[1]:.2f}), torch.sort + slice median {b[0]:.2f} us "
              f"(min {b[1]:.2f}), equal: {ok}")
        report["topk"][label] = {"ft_topk_desc_f32_us": [round(a[0], 2), round(a[1], 2)], "torch_sort_us": [round(b[0], 2), round(b[1], 2)], "equal": ok}
    print(json.dumps(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clip", action="store_true", help="the detector over a clip: per-frame loop against detect_persons_clip")
    ap.add_argument("--frames", type=int, default=32, help="--clip: frames per window")
    ap.add_argument("--rounds", type=int, default=5, help="--clip: alternations a, b")
    ap.add_argument("--nets", default="res101,vgg16", help="--clip: trunks, comma separated")
    args = ap.parse_args()
    if args.clip:
        return clip_main(args)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    anchors_np, A = proposal.generate_anchors_pre(H, W, 16)
    anchors = torch.from_numpy(anchors_np).to(dev)
    deltas = torch.from_numpy(rng.uniform(-0.5, 0.5, (int(A), 4)).astype(np.float32)).to(dev)
    scores = torch.from_numpy(rng.permutation(int(A)).astype(np.float32) / float(A)).to(dev)
    boxes = torch.empty_like(anchors)
    check(lib.ft_rpn_decode_boxes(p(anchors), p(deltas), int(A), IM_H, IM_W, p(boxes), stream))
    order = scores.sort(descending=True, stable=True)[1][:N_NMS]
    dets = torch.cat((boxes[order], scores[order, None]), 1).contiguous()
    workspace = torch.empty(lib.ft_box_nms_workspace_bytes(N_NMS), dtype=torch.uint8, device=dev)
    keep = torch.empty(N_NMS, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.ft_box_nms(p(dets), N_NMS, 0.7, 0, R, p(workspace), p(keep), p(count), stream))
    n_kept = int(count.item())
    rois = torch.zeros((R, 5), dtype=torch.float32, device=dev)
    rois[:n_kept, 1:] = dets[keep[:n_kept].long(), :4]
    rois[n_kept:, 1:] = dets[:R - n_kept, :4]

    feat = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32)).to(dev)
    nhwc32 = feat.permute(0, 2, 3, 1).contiguous()
    nhwc16 = nhwc32.half()
    pooled = torch.empty((R, C, POOLED, POOLED), dtype=torch.float32, device=dev)
    argmax = torch.empty((R, C, POOLED, POOLED), dtype=torch.int32, device=dev)
    grad_in = torch.empty_like(feat)
    s16 = 1.0 / 16
    nb = torch.stack((rois[:, 2] / 16 / (H - 1), rois[:, 1] / 16 / (W - 1), rois[:, 4] / 16 / (H - 1), rois[:, 3] / 16 / (W - 1)), 1).contiguous()
    ind = torch.zeros(R, dtype=torch.int32, device=dev)
    out16 = torch.empty((R, POOLED, POOLED, C), dtype=torch.float16, device=dev)
    out32 = torch.empty((R, POOLED, POOLED, C), dtype=torch.float32, device=dev)
    fb, ob, mask_b = feat.numel() * 4, pooled.numel() * 4, workspace.numel()
    words = (N_NMS + 63) // 64

    entries = [
        ("ft_rpn_decode_boxes A=%d" % A, int(A) * 48, lambda: lib.ft_rpn_decode_boxes(p(anchors), p(deltas), int(A), IM_H, IM_W, p(boxes), stream)),
        # the mask's tiles on or above the diagonal are written once and read at most once by the sweep
        ("ft_box_nms n=%d keep<=%d" % (N_NMS, R), N_NMS * 20 + mask_b * (words + 1) // (2 * words) * 2,
         lambda: lib.ft_box_nms(p(dets), N_NMS, 0.7, 0, R, p(workspace), p(keep), p(count), stream)),
        ("ft_box_nms n=%d no cap" % N_NMS, N_NMS * 20 + mask_b * (words + 1) // (2 * words) * 2,
         lambda: lib.ft_box_nms(p(dets), N_NMS, 0.7, 0, 0, p(workspace), p(keep), p(count), stream)),
        ("ft_roi_pool_fwd", fb + 2 * ob, lambda: lib.ft_roi_pool_fwd(p(feat), p(rois), B, C, H, W, R, s16, POOLED, POOLED, p(pooled), p(argmax), stream)),
        ("ft_roi_pool_bwd", 2 * fb + 2 * ob, lambda: lib.ft_roi_pool_bwd(p(pooled), p(rois), p(argmax), B, C, H, W, R, POOLED, POOLED, p(grad_in), stream)),
        ("ft_crop_and_resize_fwd 7x7", fb + ob, lambda: lib.ft_crop_and_resize_fwd(p(feat), p(nb), p(ind), B, C, H, W, R, POOLED, POOLED, 0.0, p(pooled), stream)),
        ("ft_crop_and_resize_bwd 7x7", 2 * fb + ob, lambda: lib.ft_crop_and_resize_bwd(p(pooled), p(nb), p(ind), B, C, H, W, R, POOLED, POOLED, p(grad_in), stream)),
        ("ft_roi_crop_nhwc_fwd fp16", fb // 2 + ob // 2, lambda: lib.ft_roi_crop_nhwc_fwd(FT_F16, p(nhwc16), p(rois), B, H, W, C, R, 16.0, POOLED, 0, p(out16), stream)),
        ("ft_roi_crop_nhwc_fwd fp16 max_pool", fb // 2 + ob // 2, lambda: lib.ft_roi_crop_nhwc_fwd(FT_F16, p(nhwc16), p(rois), B, H, W, C, R, 16.0, POOLED, 1, p(out16), stream)),
        ("ft_roi_crop_nhwc_fwd fp32", fb + ob, lambda: lib.ft_roi_crop_nhwc_fwd(FT_F32, p(nhwc32), p(rois), B, H, W, C, R, 16.0, POOLED, 0, p(out32), stream)),
    ]
    results = []
    print(f"kept {n_kept} of {N_NMS} at 0.7 (cap {R})")
    for name, nbytes, fn in entries:
        check(fn(), name)
        med, best = _time(fn, args.iters, args.warmup)
        floor = nbytes / HBM * 1e6
        results.append({"entry": name, "median_us": round(med, 2), "min_us": round(best, 2), "bytes": int(nbytes),
                        "hbm_floor_us": round(floor, 3), "floor_over_median": round(floor / med, 4)})
        print(f"{name:40s} median {med:9.2f} us  min {best:9.2f} us  {nbytes / 1e6:8.2f} MB  floor {floor:7.2f} us  = {floor / med:6.3f} of the HBM rate")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
