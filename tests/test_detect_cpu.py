"""The detector's region stage without a GPU: tests/detect_ref.py against hand-derived answers and against the golden recorded from
the reference (tests/golden/make_detect_golden.py), the decode error bound, and the refusals of every C entry (the library loads
without a GPU; a refused call launches nothing) and of the Python wrappers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_F16, FT_F32, FT_OK, FlowtrackHipError
from flowtrack.pytorch_amd.detection import ops, proposal

import detect_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_golden.npz"))
F32 = np.float32


# ---- the refs against hand-derived answers --------------------------------------------------------------------------------------
def test_iou_of_exactly_one_half_separates_the_two_comparisons():
    a, b = [0, 0, 9, 9], [0, 0, 9, 4]                  # areas 100 and 50, intersection 50: 50 / (100 + 50 - 50)
    assert R.iou(a, b) == F32(0.5) and R.iou(a, b, np.float64) == 0.5
    dets = np.array([a + [0.9], b + [0.8]], dtype=F32)
    keep, cnt = R.nms_sorted(dets, 0.5, inclusive=False)
    assert cnt == 2 and keep.tolist() == [0, 1]        # IoU > 0.5 is false: both stay
    keep, cnt = R.nms_sorted(dets, 0.5, inclusive=True)
    assert cnt == 1 and keep.tolist() == [0, -1]       # IoU >= 0.5 suppresses


def chain_boxes():
    """A suppresses B (IoU 90/110), B would suppress C (90/110), A does not reach C (80/120): C survives because B is gone."""
    return np.array([[0, 0, 9, 9, 0.9], [0, 1, 9, 10, 0.8], [0, 2, 9, 11, 0.7]], dtype=F32)


def test_suppression_chain_keeps_the_third_box():
    d = chain_boxes()
    assert R.iou(d[0, :4], d[1, :4]) > F32(0.7) and R.iou(d[1, :4], d[2, :4]) > F32(0.7) and R.iou(d[0, :4], d[2, :4]) < F32(0.7)
    keep, cnt = R.nms_sorted(d, 0.7)
    assert cnt == 2 and keep.tolist() == [0, 2, -1]
    keep, cnt = R.nms_sorted(d, 0.7, max_keep=1)
    assert cnt == 1 and keep.tolist() == [0, -1, -1]
    shuffled = d[[2, 0, 1]]
    assert R.nms(shuffled, 0.7).tolist() == [1, 0]     # indices into the unsorted input, in kept order


def test_crop_of_one_pixel_samples_the_centre():
    img = np.arange(2 * 5 * 7, dtype=F32).reshape(1, 2, 5, 7)
    out = R.crop_and_resize(img, [[0.0, 0.0, 1.0, 1.0]], [0], 1, 1)       # centre (2, 3) of the 5 x 7 map
    assert out.shape == (1, 2, 1, 1) and out[0, :, 0, 0].tolist() == [img[0, 0, 2, 3], img[0, 1, 2, 3]]
    out = R.crop_and_resize(img, [[0.0, 0.0, 0.5, 0.5]], [0], 1, 1)       # (1, 1.5): half-way between two columns
    assert out[0, 0, 0, 0] == (img[0, 0, 1, 1] + img[0, 0, 1, 2]) / 2
    out = R.crop_and_resize(img, [[0.0, 0.0, 1.0, 1.0]], [0], 5, 7)       # the identity crop
    assert np.array_equal(out[0], img[0])
    out = R.crop_and_resize(img, [[1.0, 1.0, 0.0, 0.0]], [0], 5, 7)       # a flipped box mirrors both axes
    assert np.array_equal(out[0], img[0, :, ::-1, ::-1])
    out = R.crop_and_resize(img, [[0.0, 0.0, 1.5, 1.0]], [0], 3, 1, extrapolation_value=-1.5)
    assert out[0, 0, :, 0].tolist() == [img[0, 0, 0, 3], img[0, 0, 3, 3], -1.5]   # rows 0, 3 and 6: the last one is outside
    assert not R.crop_and_resize(img, [[0.0, 0.0, 1.0, 1.0]] * 2, [-1, 1], 2, 2, extrapolation_value=9.0).any()


def test_roi_corner_rounding_is_half_away_from_zero():
    assert [R.round_half_away(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49, -0.49)] == [1, 2, 3, -1, -2, 0, 0]
    feat = np.arange(6 * 8, dtype=F32).reshape(1, 1, 6, 8)
    # scale 0.5: x1 = 5 -> 2.5 -> 3 (to-even would give 2), x2 = 9 -> 4.5 -> 5 (to-even 4); y1 = y2 = 3 -> 1.5 -> 2
    out, arg = R.roi_pool(feat, [[0, 5, 3, 9, 3]], 0.5, 1, 1)
    assert out[0, 0, 0, 0] == feat[0, 0, 2, 5] and arg[0, 0, 0, 0] == 2 * 8 + 5
    out, _ = R.roi_pool(feat, [[0, 5, 3, 5, 3]], 0.5, 1, 1)
    assert out[0, 0, 0, 0] == feat[0, 0, 2, 3]
    # -1 -> -0.5 -> -1: the bin [-1, 0] x [-1, 0] clipped to the map is the pixel (0, 0)
    out, arg = R.roi_pool(feat, [[0, -1, -1, 0, 0]], 0.5, 1, 1)
    assert out[0, 0, 0, 0] == feat[0, 0, 0, 0] and arg[0, 0, 0, 0] == 0
    # corners -0.5 and 0.5 -> -1 and 1: a 3 x 3 RoI, bins of 1.5: rows [-1, 1) and [0, 2) clipped to the map (to-even: one pixel)
    out, arg = R.roi_pool(feat, [[0, -1, -1, 1, 1]], 0.5, 2, 2)
    assert out[0, 0].tolist() == [[0.0, 1.0], [8.0, 9.0]] and arg[0, 0].tolist() == [[0, 1], [8, 9]]


def test_roi_pool_empty_bin_ties_and_foreign_images():
    feat = np.zeros((2, 1, 4, 4), dtype=F32)
    feat[0, 0, 1, 2] = feat[0, 0, 2, 1] = 5.0          # tied maxima: (1, 2) comes first in row-major order
    feat[1] = -3.0
    out, arg = R.roi_pool(feat, [[0, 0, 0, 3, 3], [1, 0, 0, 3, 3], [2, 0, 0, 3, 3], [-1, 0, 0, 3, 3], [0, 6, 6, 9, 9], [0, 3, 1, 1, 1]],
                          1.0, 1, 1)
    assert out[:, 0, 0, 0].tolist() == [5.0, -3.0, 0.0, 0.0, 0.0, 0.0] and arg[:, 0, 0, 0].tolist()[:5] == [1 * 4 + 2, 0, -1, -1, -1]
    assert arg[5, 0, 0, 0] == 1 * 4 + 3                # malformed (x2 < x1): forced to the 1 x 1 RoI at (1, 3)
    g, terms, _ = R.roi_pool_bwd(np.ones((6, 1, 1, 1), dtype=F32), [[0, 0, 0, 3, 3], [1, 0, 0, 3, 3], [2, 0, 0, 3, 3], [-1, 0, 0, 3, 3],
                                                                    [0, 6, 6, 9, 9], [0, 3, 1, 1, 1]], arg, feat.shape)
    want = np.zeros_like(feat, dtype=np.float64)
    want[0, 0, 1, 2] = want[1, 0, 0, 0] = want[0, 0, 1, 3] = 1.0          # image 1's gradient lands in image 1
    assert np.array_equal(g, want) and terms.sum() == 3


def test_max_pool_and_crop_pool_agree_with_torch():
    rng = np.random.RandomState(3)
    feat = rng.randn(2, 3, 6, 8).astype(F32)
    rois = np.array([[0, 10, 20, 90, 70], [1, 0, 0, 127, 95], [1, -20, 30, 60, 140]], dtype=F32)
    boxes, ind = R.roi_boxes(rois, 6, 8)
    crops = R.crop_and_resize(feat, boxes, ind, 14, 14)
    want = torch.nn.functional.max_pool2d(torch.from_numpy(crops), 2, 2).numpy()
    assert np.array_equal(R.max_pool_2x2(crops), want) and np.array_equal(R.crop_pool(feat, rois, max_pool=True), want)


# ---- the refs and the package's host code against the golden --------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (3, 4)])
def test_anchors_match_the_reference(h, w):
    anchors, count = proposal.generate_anchors_pre(h, w, 16)
    want = GOLDEN[f"anchors_{h}x{w}"]
    assert anchors.dtype == np.float32 and np.array_equal(anchors, want) and count == GOLDEN[f"count_{h}x{w}"] == h * w * 9
    assert np.array_equal(proposal.generate_anchors()[0], [-84.0, -40.0, 99.0, 55.0])      # 184 x 96 around (7.5, 7.5), 0-based


def test_decode_bound_holds_for_the_reference_and_is_small():
    anchors, deltas, im = GOLDEN["anchors_5x7"], GOLDEN["dec_deltas"], GOLDEN["dec_im"]
    assert np.abs(deltas[:, 2:]).max() <= 1.0 and len(anchors) == 315
    exact = R.decode_boxes(anchors, deltas, float(im[0]), float(im[1]), np.float64)
    bound = R.decode_bound(anchors, deltas)
    assert bound.max() < 1e-3, bound.max()
    for got in (GOLDEN["dec_boxes"], R.decode_boxes(anchors, deltas, F32(im[0]), F32(im[1]), F32)):
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - exact)
        print(f"decode: max err {err.max():.3e} px, max err / bound {np.max(err / bound):.3f}, bound up to {bound.max():.3e} px")
        assert np.all(err <= bound)
        hi = np.array([im[1] - 1, im[0] - 1] * 2)
        assert np.array_equal(got == 0, exact == 0) and np.array_equal(got == hi, exact == hi)     # clip edges are exact
    assert (exact == 0).any() and (exact == hi).any() and ((exact > 0) & (exact < hi)).any()


def test_proposal_ref_matches_the_reference():
    g = GOLDEN
    anchors = g["anchors_5x7"]
    blob, scores, picked = R.proposal_layer(g["prop_cls_prob"], g["prop_bbox_pred"], g["prop_im_info"], anchors, 9, int(g["prop_pre"]),
                                            int(g["prop_post"]), float(g["prop_thresh"]))
    assert blob.shape == g["prop_blob"].shape == (int(g["prop_post"]), 5) and np.array_equal(scores, g["prop_scores"])
    bound = R.decode_bound(anchors, g["prop_bbox_pred"].reshape(-1, 4))[picked]
    assert np.all(blob[:, 0] == 0) and np.all(np.abs(blob[:, 1:].astype(np.float64) - g["prop_blob"][:, 1:]) <= 2 * bound)
    assert len(np.unique(g["prop_cls_prob"][..., 9:])) == 315


# ---- refusals of the C entries (no GPU: a refused call returns before any HIP call) ------------------------------------------------
P = ctypes.c_void_p(0x1000)        # a non-NULL, 16-byte aligned stand-in: refused calls never dereference it
NULL = None


def test_box_nms_refusals(hip_lib):
    assert hip_lib.ft_box_nms_workspace_bytes(0) == 0 and hip_lib.ft_box_nms_workspace_bytes(16385) == 0
    assert hip_lib.ft_box_nms_workspace_bytes(65) == 65 * 2 * 8 and hip_lib.ft_box_nms_workspace_bytes(16384) == 16384 * 256 * 8
    assert hip_lib.ft_box_nms(NULL, 0, 0.7, 0, 0, NULL, NULL, P, None) == FT_OK                  # zero boxes
    assert hip_lib.ft_box_nms(P, -1, 0.7, 0, 0, P, P, P, None) == FT_ERR_INVALID_ARG
    assert hip_lib.ft_box_nms(P, 16385, 0.7, 0, 0, P, P, P, None) == FT_ERR_UNSUPPORTED
    assert hip_lib.ft_box_nms(P, 8, 0.7, 2, 0, P, P, P, None) == FT_ERR_INVALID_ARG             # inclusive is 0 or 1
    assert hip_lib.ft_box_nms(P, 8, float("nan"), 0, 0, P, P, P, None) == FT_ERR_INVALID_ARG
    for args in ((NULL, 8, 0.7, 0, 0, P, P, P), (P, 8, 0.7, 0, 0, NULL, P, P), (P, 8, 0.7, 0, 0, P, NULL, P), (P, 8, 0.7, 0, 0, P, P, NULL)):
        assert hip_lib.ft_box_nms(*args, None) == FT_ERR_INVALID_ARG


def test_roi_pool_refusals(hip_lib):
    fwd = lambda x, rois, B, C, H, W, Rn, ph, pw, out: hip_lib.ft_roi_pool_fwd(x, rois, B, C, H, W, Rn, 0.0625, ph, pw, out, NULL, None)
    assert fwd(NULL, NULL, 1, 8, 4, 4, 0, 7, 7, NULL) == FT_OK
    for args in ((NULL, P, 1, 8, 4, 4, 3, 7, 7, P), (P, NULL, 1, 8, 4, 4, 3, 7, 7, P), (P, P, 1, 8, 4, 4, 3, 7, 7, NULL),
                 (P, P, 0, 8, 4, 4, 3, 7, 7, P), (P, P, 1, 0, 4, 4, 3, 7, 7, P), (P, P, 1, 8, 0, 4, 3, 7, 7, P), (P, P, 1, 8, 4, -1, 3, 7, 7, P),
                 (P, P, 1, 8, 4, 4, -1, 7, 7, P), (P, P, 1, 8, 4, 4, 3, 0, 7, P), (P, P, 1, 8, 4, 4, 3, 7, 0, P)):
        assert fwd(*args) == FT_ERR_INVALID_ARG, args
    assert fwd(P, P, 1, 1024, 2048, 1024, 3, 7, 7, P) == FT_ERR_UNSUPPORTED                    # 2^31 input elements
    assert fwd(P, P, 1, 1024, 4, 4, 1 << 16, 7, 7, P) == FT_ERR_UNSUPPORTED                    # 2^31+ output elements
    bwd = hip_lib.ft_roi_pool_bwd
    assert bwd(P, P, P, 1, 8, 4, 4, 3, 7, 7, NULL, None) == FT_ERR_INVALID_ARG
    assert bwd(NULL, P, P, 1, 8, 4, 4, 3, 7, 7, P, None) == FT_ERR_INVALID_ARG
    assert bwd(P, P, NULL, 1, 8, 4, 4, 3, 7, 7, P, None) == FT_ERR_INVALID_ARG
    assert bwd(P, P, P, 1, 8, 4, 4, 3, 0, 7, P, None) == FT_ERR_INVALID_ARG
    assert bwd(P, P, P, 1, 1024, 2048, 1024, 3, 7, 7, P, None) == FT_ERR_UNSUPPORTED


def test_crop_and_resize_refusals(hip_lib):
    fwd = lambda x, boxes, ind, B, C, H, W, Rn, ch, cw, out: hip_lib.ft_crop_and_resize_fwd(x, boxes, ind, B, C, H, W, Rn, ch, cw, 0.0, out, None)
    assert fwd(NULL, NULL, NULL, 1, 8, 4, 4, 0, 7, 7, NULL) == FT_OK
    for args in ((NULL, P, P, 1, 8, 4, 4, 3, 7, 7, P), (P, NULL, P, 1, 8, 4, 4, 3, 7, 7, P), (P, P, NULL, 1, 8, 4, 4, 3, 7, 7, P),
                 (P, P, P, 1, 8, 4, 4, 3, 7, 7, NULL), (P, P, P, 0, 8, 4, 4, 3, 7, 7, P), (P, P, P, 1, 8, 4, 4, 3, 0, 7, P),
                 (P, P, P, 1, 8, 4, 4, 3, 7, -2, P), (P, P, P, 1, 8, 4, 4, -3, 7, 7, P)):
        assert fwd(*args) == FT_ERR_INVALID_ARG, args
    assert fwd(P, P, P, 2, 1024, 1024, 1024, 3, 7, 7, P) == FT_ERR_UNSUPPORTED
    bwd = hip_lib.ft_crop_and_resize_bwd
    assert bwd(P, P, P, 1, 8, 4, 4, 3, 7, 7, NULL, None) == FT_ERR_INVALID_ARG
    assert bwd(P, NULL, P, 1, 8, 4, 4, 3, 7, 7, P, None) == FT_ERR_INVALID_ARG
    assert bwd(P, P, P, 1, 8, 0, 4, 3, 7, 7, P, None) == FT_ERR_INVALID_ARG
    assert bwd(P, P, P, 2, 1024, 1024, 1024, 3, 7, 7, P, None) == FT_ERR_UNSUPPORTED


def test_roi_crop_nhwc_refusals(hip_lib):
    f = lambda dt, x, rois, B, H, W, C, Rn, stride, pooled, mp, out: hip_lib.ft_roi_crop_nhwc_fwd(dt, x, rois, B, H, W, C, Rn, stride, pooled, mp, out, None)
    assert f(FT_F16, NULL, NULL, 1, 4, 4, 8, 0, 16.0, 7, 0, NULL) == FT_OK
    for args in ((FT_F16, P, P, 1, 4, 4, 12, 3, 16.0, 7, 0, P),       # C % 8 != 0
                 (FT_F32, P, P, 1, 4, 4, 4, 3, 16.0, 7, 0, P),
                 (FT_F16, P, P, 1, 1, 4, 8, 3, 16.0, 7, 0, P),        # H < 2
                 (FT_F16, P, P, 1, 4, 1, 8, 3, 16.0, 7, 0, P),        # W < 2
                 (7, P, P, 1, 4, 4, 8, 3, 16.0, 7, 0, P),             # dtype
                 (FT_F16, NULL, P, 1, 4, 4, 8, 3, 16.0, 7, 0, P), (FT_F16, P, NULL, 1, 4, 4, 8, 3, 16.0, 7, 0, P),
                 (FT_F16, P, P, 1, 4, 4, 8, 3, 16.0, 7, 0, NULL), (FT_F16, ctypes.c_void_p(0x1008), P, 1, 4, 4, 8, 3, 16.0, 7, 0, P),
                 (FT_F16, P, P, 0, 4, 4, 8, 3, 16.0, 7, 0, P), (FT_F16, P, P, 1, 4, 4, 8, -3, 16.0, 7, 0, P),
                 (FT_F16, P, P, 1, 4, 4, 8, 3, 0.0, 7, 0, P), (FT_F16, P, P, 1, 4, 4, 8, 3, 16.0, 0, 0, P),
                 (FT_F16, P, P, 1, 4, 4, 8, 3, 16.0, 7, 2, P)):
        assert f(*args) == FT_ERR_INVALID_ARG, args
    assert f(FT_F16, P, P, 2, 1024, 1024, 1024, 3, 16.0, 7, 0, P) == FT_ERR_UNSUPPORTED
    assert f(FT_F16, P, P, 1, 4, 4, 1024, 1 << 16, 16.0, 7, 0, P) == FT_ERR_UNSUPPORTED


def test_rpn_decode_refusals(hip_lib):
    f = hip_lib.ft_rpn_decode_boxes
    assert f(NULL, NULL, 0, 600.0, 800.0, NULL, None) == FT_OK
    for args in ((NULL, P, 9, 600.0, 800.0, P), (P, NULL, 9, 600.0, 800.0, P), (P, P, 9, 600.0, 800.0, NULL), (P, P, -9, 600.0, 800.0, P),
                 (P, P, 9, 0.0, 800.0, P), (P, P, 9, 600.0, float("nan"), P), (ctypes.c_void_p(0x1004), P, 9, 600.0, 800.0, P)):
        assert f(*args, None) == FT_ERR_INVALID_ARG, args
    assert f(P, P, 1 << 29, 600.0, 800.0, P, None) == FT_ERR_UNSUPPORTED


# ---- refusals of the Python wrappers -----------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_cpu_tensors_and_wrong_ranks(hip_lib):
    feat, rois = torch.zeros(1, 8, 4, 4), torch.zeros(2, 5)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.nms(torch.zeros(4, 5), 0.7)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.RoIPoolFunction(7, 7, 1 / 16)(feat, rois)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.RoIPool(7, 7, 1 / 16)(feat, rois)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.CropAndResizeFunction(7, 7)(feat, torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.CropAndResize(7, 7)(feat, torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.RoIPoolFunction(7, 7, 1 / 16)(feat.half(), rois)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.CropAndResizeFunction(7, 7)(feat.half(), torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.nms(torch.zeros(4, 5).half(), 0.7)
    with pytest.raises(FlowtrackHipError, match="shape"):                    # wrong ranks / widths
        ops.nms(torch.zeros(4, 4), 0.7)
    with pytest.raises(FlowtrackHipError, match="shape"):
        ops.RoIPoolFunction(7, 7, 1 / 16)(feat[0], rois)
    with pytest.raises(FlowtrackHipError, match="shape"):
        ops.CropAndResizeFunction(7, 7)(feat[0], torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(FlowtrackHipError, match="shape"):
        proposal.roi_crop_nhwc(torch.zeros(4, 4, 8), rois)
    with pytest.raises(FlowtrackHipError, match="CUDA"):
        proposal.roi_crop_nhwc(torch.zeros(1, 4, 4, 8), rois)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        proposal.proposal_layer(torch.zeros(1, 5, 7, 18), torch.zeros(1, 5, 7, 36), (80.0, 112.0, 1.0), "TEST", 16, GOLDEN["anchors_5x7"], 9)
    with pytest.raises(FlowtrackHipError, match="cfg_key"):
        proposal.proposal_layer(torch.zeros(1, 5, 7, 18), torch.zeros(1, 5, 7, 36), (80.0, 112.0, 1.0), "VAL", 16, GOLDEN["anchors_5x7"], 9)
    assert proposal.RPN_DEFAULTS == {"TEST": (6000, 300, 0.7), "TRAIN": (12000, 2000, 0.7)}


