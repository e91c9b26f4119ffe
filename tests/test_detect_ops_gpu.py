"""The detector's region-stage kernels on the GPU (csrc/detect_ops.hip) against tests/detect_ref.py: integer-equal keep lists,
bit-equal forward values (compared as bit patterns, so a zero's sign counts), exact-sum gradients bit for bit and one float
gradient per operator within the derived summation bound; the decode within its derived bound against the golden's inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from flowtrack.pytorch_amd.detection import ops, proposal

import detect_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_golden.npz"))
F32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


# ---- NMS ------------------------------------------------------------------------------------------------------------------------
def nms_case(n, seed):
    """n integer-coordinate boxes in score-descending order: a few tight clusters (many suppressions, many IoUs that are ratios of
    small integers), and — where n allows — a pair at IoU exactly 1/2 and a chain A -> B -> C, all shuffled among the others."""
    rng = np.random.RandomState(seed)
    special = [[100, 100, 109, 109], [100, 100, 109, 104],                    # 50 / (100 + 50 - 50)
               [200, 200, 209, 209], [200, 203, 209, 212], [200, 206, 209, 215]]  # 70 / 130, 70 / 130, 40 / 160
    boxes = special[:min(n, 5)] if n >= 2 else []
    centres = rng.randint(10, 60, (6, 2))
    while len(boxes) < n:
        cx, cy = centres[rng.randint(len(centres))] + rng.randint(-2, 3, 2)
        w, h = rng.randint(4, 12, 2)
        boxes.append([cx - w // 2, cy - h // 2, cx - w // 2 + w - 1, cy - h // 2 + h - 1])
    boxes = np.array(boxes, dtype=F32)
    order = rng.permutation(n)
    if n >= 5:                                           # the five special boxes keep their relative (score) order
        pos = np.sort(rng.choice(n, 5, replace=False))
        order[pos] = np.arange(5)
        order[np.setdiff1d(np.arange(n), pos)] = 5 + rng.permutation(n - 5)
    scores = (1.0 - np.arange(n) / (n + 1.0)).astype(F32)
    return np.concatenate((boxes[order], scores[:, None]), 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 200])
def test_box_nms_matches_the_reference_sweep(hip_lib, n):
    dets = nms_case(n, 100 + n)
    d = _dev(dets)
    for inclusive in (False, True):
        want_keep, want_cnt = R.nms_sorted(dets, 0.5, inclusive)
        keep, count = ops.box_nms_sorted(d, 0.5, inclusive=inclusive)
        print(f"n={n} inclusive={inclusive}: kept {want_cnt}")
        assert int(count.item()) == want_cnt and np.array_equal(keep.cpu().numpy(), want_keep)
        for cap in sorted({1, max(1, want_cnt // 2), want_cnt, want_cnt + 3}):
            want_keep_c, want_cnt_c = R.nms_sorted(dets, 0.5, inclusive, cap)
            keep, count = ops.box_nms_sorted(d, 0.5, inclusive=inclusive, max_keep=cap)
            assert want_cnt_c == min(cap, want_cnt) and int(count.item()) == want_cnt_c
            assert np.array_equal(keep.cpu().numpy(), want_keep_c) and np.all(want_keep_c[want_cnt_c:] == -1)
    if n >= 5:
        find = lambda box: int(np.nonzero((dets[:, :4] == box).all(1))[0][0])
        keep_gt, keep_ge = R.nms_sorted(dets, 0.5, False)[0].tolist(), R.nms_sorted(dets, 0.5, True)[0].tolist()
        half = find([100, 100, 109, 104])                # IoU exactly 1/2 with its partner: `>` keeps it, `>=` does not
        assert half in keep_gt and half not in keep_ge
        assert find([200, 206, 209, 215]) in keep_gt and find([200, 203, 209, 212]) not in keep_gt   # C survives: B was suppressed
    want_keep, want_cnt = R.nms_sorted(dets, 0.7, False)
    keep, count = ops.box_nms_sorted(d, 0.7)
    assert int(count.item()) == want_cnt and np.array_equal(keep.cpu().numpy(), want_keep)


# ---- RoI pooling ----------------------------------------------------------------------------------------------------------------
ROI_MAP = (2, 5, 9, 11)


def roi_cases(scale):
    """(batch, x1, y1, x2, y2) in feature cells, returned in image pixels for `scale` (both scales make the products exact)."""
    cells = [(0, 0, 0, 10, 8),            # the full map
             (0, 3, 4, 3, 4),             # a single pixel
             (0, 6, 2, 3, 5),             # malformed: x2 < x1
             (0, -3, -2, 4, 3), (0, 8, 6, 14, 12),       # partly outside
             (0, 13, 10, 16, 12), (0, -8, -8, -3, -3),   # wholly outside
             (0, 2, 2, 3, 3),             # narrower than the pooled grid
             (0, 1.5, 2.5, 6.5, 5.5), (0, -0.5, -1.5, 4.5, 3.5), (1, 0.5, 0.5, 9.5, 7.5),   # half-way roundings
             (1, 0, 0, 10, 8), (1, 2, 1, 7, 6),          # image 1
             (-1, 0, 0, 10, 8), (2, 0, 0, 10, 8)]        # no such image
    rois = np.array(cells, dtype=np.float64)
    rois[:, 1:] /= scale
    assert np.array_equal(rois.astype(F32)[:, 1:] * F32(scale), np.array(cells, dtype=F32)[:, 1:])
    return rois.astype(F32)


def roi_features(kind):
    rng = np.random.RandomState(11)
    if kind == "tied":
        return rng.randint(-3, 4, ROI_MAP).astype(F32)   # seven values over 99 pixels: every bin has tied maxima
    return rng.randn(*ROI_MAP).astype(F32)


@pytest.mark.parametrize("kind", ["float", "tied"])
@pytest.mark.parametrize("scale", [1.0 / 16, 0.5])
@pytest.mark.parametrize("ph,pw", [(7, 7), (1, 1), (2, 3)])
def test_roi_pool_forward_and_backward(hip_lib, ph, pw, scale, kind):
    feat, rois = roi_features(kind), roi_cases(scale)
    B, C, H, W = feat.shape
    Rn = len(rois)
    want, want_arg = R.roi_pool(feat, rois, scale, ph, pw)
    assert (want_arg == -1).any() and (want_arg[11:13] >= 0).all()
    d_feat, d_rois = _dev(feat), _dev(rois)
    out = torch.full((Rn, C, ph, pw), 7.0, device="cuda")
    arg = torch.full((Rn, C, ph, pw), 7, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.ft_roi_pool_fwd(_ptr(d_feat), _ptr(d_rois), B, C, H, W, Rn, scale, ph, pw, _ptr(out), _ptr(arg), stream) == 0
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and np.array_equal(arg.cpu().numpy(), want_arg)
    out2 = torch.full_like(out, 7.0)                      # the arg-max is optional in forward
    assert hip_lib.ft_roi_pool_fwd(_ptr(d_feat), _ptr(d_rois), B, C, H, W, Rn, scale, ph, pw, _ptr(out2), None, stream) == 0
    assert torch.equal(out2, out)
    rng = np.random.RandomState(5)
    for exact in (True, False):
        go = rng.randint(-4, 5, want.shape).astype(F32) if exact else rng.randn(*want.shape).astype(F32)
        g_want, terms, mag = R.roi_pool_bwd(go, rois, want_arg, feat.shape)
        g = torch.full(ROI_MAP, 7.0, device="cuda")
        assert hip_lib.ft_roi_pool_bwd(_ptr(_dev(go)), _ptr(d_rois), _ptr(arg), B, C, H, W, Rn, ph, pw, _ptr(g), stream) == 0
        got = g.cpu().numpy()
        assert terms.max() > 1 and (terms[1] > 0).any()   # several RoIs meet on one element; image 1 gets its own gradient
        if exact:
            assert np.array_equal(_bits(got + F32(0)), _bits(g_want.astype(F32) + F32(0)))
        else:
            err, bound = np.abs(got.astype(np.float64) - g_want), R.sum_bound(terms, mag)
            print(f"roi_pool bwd float: max err {err.max():.3e}, max bound {bound.max():.3e}, up to {terms.max()} terms")
            assert np.all(err <= bound) and np.all(got[terms == 0] == 0)


# ---- crop_and_resize ------------------------------------------------------------------------------------------------------------
CROP_IMAGE = (2, 3, 6, 8)
CROP_BOXES = np.array([[0.1, 0.2, 0.7, 0.9],            # inside
                       [0.25, 0.5, 1.0, 1.0],           # ends exactly on the last row / column
                       [-0.3, -0.2, 0.6, 1.3],          # partly outside
                       [0.9, 0.8, 0.1, 0.2],            # flipped
                       [0.0, 0.0, 1.0, 1.0],
                       [1.2, 1.1, 1.5, 1.6],            # wholly outside
                       [0.1, 0.2, 0.7, 0.9], [0.1, 0.2, 0.7, 0.9]], dtype=F32)
CROP_IND = np.array([0, 1, 0, 1, 1, 0, -1, 2], dtype=np.int32)


def _crop_fwd(lib, image, boxes, ind, ch, cw, extrapolation):
    B, C, H, W = image.shape
    out = torch.full((len(boxes), C, ch, cw), 7.0, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ft_crop_and_resize_fwd(_ptr(_dev(image)), _ptr(_dev(boxes)), _ptr(_dev(ind)), B, C, H, W, len(boxes), ch, cw, extrapolation,
                                      _ptr(out), stream) == 0
    return out.cpu().numpy()


def _crop_bwd(lib, go, boxes, ind, shape):
    B, C, H, W = shape
    g = torch.full(shape, 7.0, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ft_crop_and_resize_bwd(_ptr(_dev(go)), _ptr(_dev(boxes)), _ptr(_dev(ind)), B, C, H, W, len(boxes), go.shape[2], go.shape[3],
                                      _ptr(g), stream) == 0
    return g.cpu().numpy()


@pytest.mark.parametrize("extrapolation", [0.0, -1.5])
@pytest.mark.parametrize("ch,cw", [(7, 7), (14, 14), (1, 1), (2, 5)])
def test_crop_and_resize_forward_is_bit_exact(hip_lib, ch, cw, extrapolation):
    image = np.random.RandomState(21).randn(*CROP_IMAGE).astype(F32)
    want = R.crop_and_resize(image, CROP_BOXES, CROP_IND, ch, cw, extrapolation)
    got = _crop_fwd(hip_lib, image, CROP_BOXES, CROP_IND, ch, cw, extrapolation)
    assert np.array_equal(_bits(got), _bits(want))
    assert not got[6:].any() and np.all(got[5] == F32(extrapolation))
    if ch > 1:
        assert (got[2] == F32(extrapolation)).any() and (got[2] != F32(extrapolation)).any()
    if (ch, cw) in ((7, 7), (2, 5)):                      # steps of 0.625 / 3.75 rows and 0.583.. / 0.875 columns: exact in fp32 where it matters
        assert np.array_equal(got[1, :, -1, -1], image[1, :, 5, 7])      # the last sample sits on the last pixel


def test_crop_and_resize_backward(hip_lib):
    rng = np.random.RandomState(22)
    # exact: crop (3, 5) on the 6 x 8 image with boxes whose steps are 2.5 / 1.25 rows and 1.75 / 3.5 columns
    boxes = np.array([[0, 0, 1, 1], [1, 1, 0, 0], [0.5, 0, 1, 2], [-0.5, -1, 0.5, 1], [0, 0, 1, 1], [0, 0, 1, 1]], dtype=F32)
    ind = np.array([0, 1, 1, 0, 2, -1], dtype=np.int32)
    for b in boxes:
        for lerp in (R.crop_axis(b[0], b[2], 3, 6)[3], R.crop_axis(b[1], b[3], 5, 8)[3]):
            assert np.array_equal(lerp * 4, np.round(lerp * 4))          # the premise: every lerp is a multiple of 1/4
    go = rng.randint(-4, 5, (len(boxes), 3, 3, 5)).astype(F32)
    want, terms, _ = R.crop_and_resize_bwd(go, boxes, ind, CROP_IMAGE)
    got = _crop_bwd(hip_lib, go, boxes, ind, CROP_IMAGE)
    assert terms.max() > 4 and (terms == 0).any()
    assert np.array_equal(_bits(got + F32(0)), _bits(want.astype(F32) + F32(0)))
    # float: every term is a product formed with four roundings, the sum runs in any order
    go = rng.randn(len(CROP_BOXES), 3, 7, 7).astype(F32)
    want, terms, mag = R.crop_and_resize_bwd(go, CROP_BOXES, CROP_IND, CROP_IMAGE)
    got = _crop_bwd(hip_lib, go, CROP_BOXES, CROP_IND, CROP_IMAGE)
    err, bound = np.abs(got.astype(np.float64) - want), R.sum_bound(terms, mag, per_term_roundings=4)
    print(f"crop_and_resize bwd float: max err {err.max():.3e}, max bound {bound.max():.3e}, up to {terms.max()} terms")
    assert np.all(err <= bound)


# ---- the fused NHWC form --------------------------------------------------------------------------------------------------------
def nhwc_rois(Rn, H, W, stride=16.0):
    rng = np.random.RandomState(31 + Rn)
    x1, y1 = rng.uniform(-20, W * stride * 0.7, Rn), rng.uniform(-20, H * stride * 0.7, Rn)
    rois = np.stack((rng.randint(0, 2, Rn), x1, y1, x1 + rng.uniform(4, W * stride * 0.8, Rn), y1 + rng.uniform(4, H * stride * 0.8, Rn)), 1)
    rois[0] = (1, 0, 0, (W - 1) * stride, (H - 1) * stride)             # the whole map of image 1: the last sample is the last pixel
    if Rn > 4:
        rois[3, 0], rois[4, 0] = 2, -1                                  # no such image
    return rois.astype(F32)


@pytest.mark.parametrize("Rn", [1, 37])
@pytest.mark.parametrize("max_pool", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [8, 136])
def test_roi_crop_nhwc_matches_crop_pool_layer(hip_lib, C, dtype, max_pool, Rn):
    B, H, W = 2, 5, 7
    feat = np.random.RandomState(C).randn(B, C, H, W).astype(F32)
    if dtype == torch.float16:
        feat = feat.astype(np.float16).astype(F32)
    rois = nhwc_rois(Rn, H, W)
    want = R.crop_pool(feat, rois, 16.0, 7, max_pool).transpose(0, 2, 3, 1)       # fp32 restatement, NHWC
    d_rois = _dev(rois)
    nhwc = _dev(feat).permute(0, 2, 3, 1).contiguous().to(dtype)
    got = proposal.roi_crop_nhwc(nhwc, d_rois, 16.0, 7, max_pool)
    assert got.shape == (Rn, 7, 7, C) and got.dtype == dtype and got.is_contiguous()
    if dtype == torch.float32:
        layer = proposal.crop_pool_layer(_dev(feat), d_rois, max_pool).permute(0, 2, 3, 1).contiguous()
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(layer.cpu().numpy()))
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(np.ascontiguousarray(want)))
    else:
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(np.ascontiguousarray(want).astype(np.float16)))   # rounded once
    if not max_pool:
        assert np.array_equal(got[0, 6, 6].float().cpu().numpy(), feat[1, :, H - 1, W - 1])      # the last sample is the last pixel
    if Rn > 4:
        assert not got[3:5].any() and got[5].any()


# ---- RPN decode -----------------------------------------------------------------------------------------------------------------
def test_rpn_decode_within_the_derived_bound(hip_lib):
    anchors, deltas, im = GOLDEN["anchors_5x7"], GOLDEN["dec_deltas"], GOLDEN["dec_im"]
    got = proposal.decode_boxes(_dev(anchors), _dev(deltas), float(im[0]), float(im[1])).cpu().numpy()
    exact = R.decode_boxes(anchors, deltas, float(im[0]), float(im[1]), np.float64)
    bound = R.decode_bound(anchors, deltas)
    err = np.abs(got.astype(np.float64) - exact)
    print(f"decode: max err {err.max():.3e} px, max err / bound {np.max(err / bound):.3f}, bound up to {bound.max():.3e} px")
    assert np.all(err <= bound)
    hi = np.array([im[1] - 1, im[0] - 1] * 2)
    assert np.array_equal(got == 0, exact == 0) and np.array_equal(got == hi, exact == hi) and (exact == 0).any() and (exact == hi).any()
    assert np.all(np.abs(got.astype(np.float64) - GOLDEN["dec_boxes"]) <= 2 * bound)
