"""The four glue kernels of the detector network (csrc/detect_net_ops.hip) alone, each against its float64 reference
(tests/detect_net_ref.py) within its derived bound, plus the exact cases, the refusals and the zero-row calls."""
import ctypes
import os

import numpy as np
import pytest
import torch

import detect_net_ref as R
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_F16, FT_F32, FT_OK

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "detect_net_golden.npz"), allow_pickle=False)
SEED, TARGET, MAX_SIZE = int(G["seed"]), int(G["target_size"]), int(G["max_size"])
MEANS = (ctypes.c_double * 3)(*R.PIXEL_MEANS)
STDS4, MEANS4 = (ctypes.c_float * 4)(*R.BBOX_STDS), (ctypes.c_float * 4)(*R.BBOX_MEANS)
CODE = {torch.float16: FT_F16, torch.float32: FT_F32}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _blob(lib, frame, Hb, Wb, sy, sx):
    f = torch.from_numpy(frame).cuda()
    out = torch.full((1, 3, Hb, Wb), float("nan"), device="cuda")
    assert lib.ft_detect_blob_fwd(_p(f), frame.shape[0], frame.shape[1], MEANS, Hb, Wb, sy, sx, _p(out), _stream()) == FT_OK
    return out.cpu().numpy()


@pytest.mark.parametrize("case", ("a", "b"))
def test_blob_golden_cases(hip_lib, case):
    h, w = (int(v) for v in G[case + "_frame_hw"])
    frame = synth.detector_frame(SEED, h, w)
    im_scale, Hb, Wb = R.blob_size(h, w, TARGET, MAX_SIZE)
    got = _blob(hip_lib, frame, Hb, Wb, 1.0 / im_scale, 1.0 / im_scale)
    want = R.blob_ref(frame, R.PIXEL_MEANS, Hb, Wb, 1.0 / im_scale, 1.0 / im_scale, np.float64)
    err, bound = np.abs(got - want).max(), R.blob_bound(frame, R.PIXEL_MEANS)
    print(f"blob {case}: {h}x{w} -> {Hb}x{Wb}, max abs vs float64 {err:.3e}, bound {bound:.3e}; vs the golden {np.abs(got - G[case + '_blob']).max():.3e}")
    assert err <= bound
    assert np.abs(got - G[case + "_blob"]).max() <= bound + 2.0 ** -24 * np.abs(G[case + "_blob"]).max()   # (the golden is the float64 form rounded)
    assert np.array_equal(got, R.blob_ref(frame, R.PIXEL_MEANS, Hb, Wb, 1.0 / im_scale, 1.0 / im_scale, np.float32))


def test_blob_upscale_hits_both_borders(hip_lib):
    frame = synth.detector_frame(SEED + 1, 3, 5)
    got = _blob(hip_lib, frame, 7, 11, 3.0 / 7.0, 5.0 / 11.0)
    want = R.blob_ref(frame, R.PIXEL_MEANS, 7, 11, 3.0 / 7.0, 5.0 / 11.0, np.float64)
    src = (frame.astype(np.float64) - R.PIXEL_MEANS).astype(np.float32).transpose(2, 0, 1)
    assert np.abs(got - want).max() <= R.blob_bound(frame, R.PIXEL_MEANS)
    # output 0 samples left of / above pixel 0 and output n - 1 at or past the last pixel: weight zeroed, index clamped
    assert np.array_equal(got[0, :, 0, 0], src[:, 0, 0]) and np.array_equal(got[0, :, -1, -1], src[:, -1, -1])
    assert np.array_equal(got[0, :, 0, -1], src[:, 0, -1]) and np.array_equal(got[0, :, -1, 0], src[:, -1, 0])


def test_blob_scale_one_is_the_identity(hip_lib):
    frame = synth.detector_frame(SEED + 2, 37, 53)
    got = _blob(hip_lib, frame, 37, 53, 1.0, 1.0)
    want = (frame.astype(np.float64) - R.PIXEL_MEANS).astype(np.float32).transpose(2, 0, 1)[None]
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32))


def _rpn_softmax(lib, x, A, cstride=None, coff=0):
    rows = x.shape[0]
    buf = x
    if cstride is not None:
        buf = torch.full((rows, cstride), 7.0, dtype=x.dtype, device="cuda")
        buf[:, coff:coff + 2 * A] = x
    out = torch.full((rows, 2 * A), float("nan"), device="cuda")
    assert lib.ft_rpn_softmax_fwd(CODE[x.dtype], _p(buf), rows, A, buf.shape[1], coff, _p(out), _stream()) == FT_OK
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("fp32", "fp16"))
@pytest.mark.parametrize("A,rows", ((9, 35), (1, 300)))
def test_rpn_softmax(hip_lib, dtype, A, rows):
    x = synth.normal(SEED, f"rpn_sm{A}", (rows, 2 * A), std=3.0)
    x[0], x[1, :A], x[1, A:], x[2, :A], x[2, A:] = 1.25, 60.0, -60.0, -60.0, 60.0
    x = x.to(dtype).cuda()
    xin = x.float().cpu().numpy()
    want, bound = R.rpn_softmax_ref(xin, A, np.float64), R.softmax_bound(xin.reshape(-1, 2, A), 1).reshape(-1, 2 * A)
    for cstride, coff in ((None, 0), (64, 8)):
        got = _rpn_softmax(hip_lib, x, A, cstride, coff)
        print(f"rpn softmax A={A} {dtype} cstride {cstride}: max abs {np.abs(got - want).max():.3e}, bound {bound.max():.3e}")
        assert np.isfinite(got).all() and np.all(np.abs(got - want) <= bound)
        assert np.all(got[0] == 0.5)
        assert np.all(got[1, :A] == 1.0) and np.all(got[1, A:] <= 1e-37) and np.all(got[2, A:] == 1.0)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("fp32", "fp16"))
@pytest.mark.parametrize("C", (8, 2048))
def test_mean_pool(hip_lib, dtype, C):
    x = synth.normal(SEED, f"mp{C}", (3, 7, 7, C), std=2.0).to(dtype).cuda()
    out = torch.full((3, C), float("nan"), dtype=dtype, device="cuda")
    assert hip_lib.ft_rcnn_mean_pool_fwd(CODE[dtype], _p(x), 3, 7, C, _p(out), _stream()) == FT_OK
    xin = x.float().cpu().numpy()
    got, want = out.float().cpu().numpy().astype(np.float64), R.mean_pool_ref(xin, np.float64)
    bound = R.mean_pool_bound(xin, np.float16 if dtype == torch.float16 else np.float32)
    print(f"mean pool C={C} {dtype}: max abs {np.abs(got - want).max():.3e}, largest bound {bound.max():.3e}")
    assert np.all(np.abs(got - want) <= bound)
    # multiples of 49: every row sum, row mean, their sum and the final mean are integers: bit for bit in either dtype
    xi = (49.0 * torch.floor(synth.uniform(SEED, f"mpi{C}", (3, 7, 7, C), -20, 21))).to(dtype).cuda()
    assert hip_lib.ft_rcnn_mean_pool_fwd(CODE[dtype], _p(xi), 3, 7, C, _p(out), _stream()) == FT_OK
    exact = R.mean_pool_ref(xi.float().cpu().numpy(), np.float64)
    assert np.array_equal(exact, np.round(exact)) and np.array_equal(out.float().cpu().numpy().astype(np.float64), exact)


def _detections(lib, score, raw, rois, im_scale, im_h, im_w, outs=(True, True, True)):
    """An input that no requested output reads is passed as NULL, as the header allows."""
    R_, K = score.shape
    ts = torch.from_numpy(np.ascontiguousarray(score)).cuda() if outs[0] else None
    tr = torch.from_numpy(np.ascontiguousarray(raw)).cuda() if outs[1] or outs[2] else None
    to = torch.from_numpy(np.ascontiguousarray(rois)).cuda() if outs[2] else None
    prob = torch.full((R_, K), float("nan"), device="cuda") if outs[0] else None
    deltas = torch.full((R_, 4 * K), float("nan"), device="cuda") if outs[1] else None
    boxes = torch.full((R_, 4 * K), float("nan"), device="cuda") if outs[2] else None
    st = lib.ft_rcnn_detections_fwd(_p(ts), _p(tr), _p(to), R_, K, STDS4, MEANS4, im_scale, im_h, im_w, _p(prob), _p(deltas), _p(boxes), _stream())
    assert st == FT_OK
    return tuple(None if t is None else t.cpu().numpy() for t in (prob, deltas, boxes))


def _detection_inputs(R_, K):
    score = synth.normal(SEED, f"det_s{R_}_{K}", (R_, K), std=2.0).numpy()
    raw = synth.uniform(SEED, f"det_d{R_}_{K}", (R_, 4 * K), -4.0, 4.0).numpy()
    xy = synth.uniform(SEED, f"det_r{R_}_{K}", (R_, 4), 0.0, 1.0).numpy()
    rois = np.zeros((R_, 5), dtype=np.float32)
    rois[:, 1], rois[:, 2] = 300.0 * xy[:, 0], 200.0 * xy[:, 1]
    rois[:, 3], rois[:, 4] = rois[:, 1] + 5.0 + 150.0 * xy[:, 2], rois[:, 2] + 5.0 + 120.0 * xy[:, 3]
    return score, raw, rois


@pytest.mark.parametrize("K", (1, 3, 81))
@pytest.mark.parametrize("R_", (1, 41))
def test_detections(hip_lib, R_, K):
    score, raw, rois = _detection_inputs(R_, K)
    im_scale, im_h, im_w = 125.0 / 96.0, 240.0, 320.0
    want = R.detections_ref(score, raw, rois, R.BBOX_STDS, R.BBOX_MEANS, np.float32(im_scale), im_h, im_w, np.float64)
    got = _detections(hip_lib, score, raw, rois, im_scale, im_h, im_w)
    b_prob, b_box = R.softmax_bound(score, 1), R.detections_bound(raw, rois, R.BBOX_STDS, R.BBOX_MEANS, np.float32(im_scale))
    print(f"detections R={R_} K={K}: prob {np.abs(got[0] - want[0]).max():.3e} (bound {b_prob.max():.3e}), boxes "
          f"{np.abs(got[2] - want[2]).max():.3e} (largest bound {b_box.max():.3e})")
    assert np.all(np.abs(got[0] - want[0]) <= b_prob)
    assert np.array_equal(got[1], want[1])                       # two fp32 operations, rounded separately: the same bits
    assert np.all(np.abs(got[2] - want[2]) <= b_box)
    # each output skipped in turn; without pred_boxes the call gets rois = NULL (and cls_score = NULL without cls_prob)
    for outs in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (False, True, False), (True, False, False)):
        part = _detections(hip_lib, score, raw, rois, im_scale, im_h, im_w, outs)
        for on, g_, full in zip(outs, part, got):
            assert (g_ is None) if not on else np.array_equal(g_, full)


def test_detections_clip_is_one_sided(hip_lib):
    """model/test.py:69-79: x1 / y1 are only raised to 0 and x2 / y2 only lowered to the frame's last pixel.  A box decoded right
    of the frame keeps its x1 beyond im_w - 1 (and gets x2 = im_w - 1 < x1), one decoded left of it keeps its negative x2."""
    rois = np.array([[0, 290, 10, 318, 60], [0, 2, 150, 30, 198]], dtype=np.float32)
    raw = np.zeros((2, 4), dtype=np.float32)
    raw[0, 0], raw[1, 0], raw[1, 1] = 20.0, -30.0, 25.0          # dx = 2 widths to the right; 3 to the left, dy 2.5 heights down
    got = _detections(hip_lib, np.zeros((2, 1), np.float32), raw, rois, 1.0, 200.0, 320.0)
    want = R.detections_ref(np.zeros((2, 1), np.float32), raw, rois, R.BBOX_STDS, R.BBOX_MEANS, 1.0, 200.0, 320.0, np.float64)
    assert np.all(np.abs(got[2] - want[2]) <= R.detections_bound(raw, rois, R.BBOX_STDS, R.BBOX_MEANS, 1.0))
    assert got[2][0, 0] > 319.0 and got[2][0, 2] == 319.0 and got[2][1, 2] < 0.0 and got[2][1, 0] == 0.0
    assert got[2][1, 1] > 199.0 and got[2][1, 3] == 199.0 and np.all(got[0] == 1.0)


def test_zero_rows_and_refusals(hip_lib):
    lib, s = hip_lib, _stream()
    sentinel = torch.full((64,), 3.0, device="cuda")
    p, u8 = _p(sentinel), _p(torch.zeros(64, dtype=torch.uint8, device="cuda"))
    # zero rows: FT_OK, nothing launched (NULL pointers are never touched)
    assert lib.ft_detect_blob_fwd(None, 4, 4, MEANS, 0, 5, 1.0, 1.0, None, s) == FT_OK
    assert lib.ft_rpn_softmax_fwd(FT_F32, None, 0, 9, 18, 0, None, s) == FT_OK
    assert lib.ft_rcnn_mean_pool_fwd(FT_F16, None, 0, 7, 2048, None, s) == FT_OK
    assert lib.ft_rcnn_detections_fwd(None, None, None, 0, 3, STDS4, MEANS4, 1.0, 10.0, 10.0, None, None, None, s) == FT_OK
    # refusals
    assert lib.ft_detect_blob_fwd(None, 4, 4, MEANS, 4, 4, 1.0, 1.0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_detect_blob_fwd(u8, 4, 4, None, 4, 4, 1.0, 1.0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_detect_blob_fwd(u8, 4, 4, MEANS, 4, 4, 0.0, 1.0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_detect_blob_fwd(u8, -1, 4, MEANS, 4, 4, 1.0, 1.0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_detect_blob_fwd(u8, 4, 4, MEANS, 30000, 30000, 1.0, 1.0, p, s) == FT_ERR_UNSUPPORTED
    assert lib.ft_rpn_softmax_fwd(5, p, 1, 9, 18, 0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rpn_softmax_fwd(FT_F32, p, 1, 0, 18, 0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rpn_softmax_fwd(FT_F32, p, 1, 9, 17, 0, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rpn_softmax_fwd(FT_F32, p, 1, 9, 18, 0, None, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rpn_softmax_fwd(FT_F32, p, 1, (1 << 30) + 9, 18, 0, p, s) == FT_ERR_INVALID_ARG     # 2 A does not fit an int
    assert lib.ft_rpn_softmax_fwd(FT_F32, p, 1 << 31, 1, 2, 0, p, s) == FT_ERR_UNSUPPORTED
    assert lib.ft_rcnn_mean_pool_fwd(FT_F32, p, 1, 7, 12, p, s) == FT_ERR_INVALID_ARG          # C % 8
    assert lib.ft_rcnn_mean_pool_fwd(FT_F32, p, 1, 0, 8, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_mean_pool_fwd(FT_F32, ctypes.c_void_p(sentinel.data_ptr() + 4), 1, 1, 8, p, s) == FT_ERR_INVALID_ARG     # alignment
    assert lib.ft_rcnn_mean_pool_fwd(FT_F32, p, 1 << 20, 7, 2048, p, s) == FT_ERR_UNSUPPORTED
    assert lib.ft_rcnn_detections_fwd(p, p, p, 1, 0, STDS4, MEANS4, 1.0, 10.0, 10.0, p, p, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_detections_fwd(p, p, p, 1, 3, STDS4, MEANS4, 0.0, 10.0, 10.0, p, p, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_detections_fwd(p, p, p, 1, 3, None, MEANS4, 1.0, 10.0, 10.0, p, p, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_detections_fwd(None, p, p, 1, 3, STDS4, MEANS4, 1.0, 10.0, 10.0, p, None, None, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_detections_fwd(p, p, None, 1, 3, STDS4, MEANS4, 1.0, 10.0, 10.0, None, None, p, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_detections_fwd(p, None, p, 1, 3, STDS4, MEANS4, 1.0, 10.0, 10.0, None, p, None, s) == FT_ERR_INVALID_ARG
    assert lib.ft_rcnn_detections_fwd(p, p, p, 1 << 26, 81, STDS4, MEANS4, 1.0, 10.0, 10.0, p, p, p, s) == FT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(sentinel == 3.0)                            # a refused call launches nothing
