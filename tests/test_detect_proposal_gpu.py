"""The detector's region stage through its Python surface on the GPU (detection/ops.py, detection/proposal.py): the proposal layer
against the golden recorded from the reference, the autograd drop-ins through loss.backward(), nms() on unsorted boxes, and the
layout claim of the fused NHWC form (its output is an ft_conv2d_fwd input as it stands)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd._lib import FT_F16, FT_LAYOUT_NHWC, ConvDesc, FlowtrackHipError
from flowtrack.pytorch_amd.detection import ops, proposal
from flowtrack.pytorch_amd.hip_ops import pack_conv_weights

import detect_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_golden.npz"))
F32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def test_proposal_layer_matches_the_reference(hip_lib):
    g = GOLDEN
    anchors, pre, post, thresh = g["anchors_5x7"], int(g["prop_pre"]), int(g["prop_post"]), float(g["prop_thresh"])
    blob, scores = proposal.proposal_layer(_dev(g["prop_cls_prob"]), _dev(g["prop_bbox_pred"]), g["prop_im_info"], "TEST", 16, _dev(anchors), 9,
                                           pre_nms_topN=pre, post_nms_topN=post, nms_thresh=thresh)
    blob, scores = blob.cpu().numpy(), scores.cpu().numpy()
    assert blob.shape == g["prop_blob"].shape == (post, 5) and blob.dtype == np.float32
    assert np.array_equal(scores.view(np.uint32), g["prop_scores"].view(np.uint32))      # distinct scores: the same set, the same order
    _, _, picked = R.proposal_layer(g["prop_cls_prob"], g["prop_bbox_pred"], g["prop_im_info"], anchors, 9, pre, post, thresh)
    deltas = g["prop_bbox_pred"].reshape(-1, 4)
    exact = R.decode_boxes(anchors, deltas, float(g["prop_im_info"][0]), float(g["prop_im_info"][1]), np.float64)[picked]
    bound = R.decode_bound(anchors, deltas)[picked]
    err = np.abs(blob[:, 1:].astype(np.float64) - exact)
    print(f"proposal_layer: kept {len(blob)}, max coordinate err {err.max():.3e} px, bound up to {bound.max():.3e} px")
    assert np.all(blob[:, 0] == 0) and np.all(err <= bound)
    assert np.all(np.abs(blob[:, 1:].astype(np.float64) - g["prop_blob"][:, 1:]) <= 2 * bound)
    # the cfg_key defaults (6000 / 300 / 0.7 here: no cut before, none after) through the numpy-anchors path
    blob_all, scores_all = proposal.proposal_layer(_dev(g["prop_cls_prob"]), _dev(g["prop_bbox_pred"]), g["prop_im_info"], b"TEST", 16, anchors, 9)
    want_blob, want_scores, _ = R.proposal_layer(g["prop_cls_prob"], g["prop_bbox_pred"], g["prop_im_info"], anchors, 9, 6000, 300, 0.7)
    assert np.array_equal(scores_all.cpu().numpy(), want_scores) and len(want_scores) > post and blob_all.shape == want_blob.shape


def test_nms_on_unsorted_boxes(hip_lib):
    rng = np.random.RandomState(41)
    n = 150
    c = rng.randint(0, 40, (n, 2))
    wh = rng.randint(5, 25, (n, 2))
    dets = np.concatenate((c, c + wh - 1, rng.permutation(n)[:, None] / n), 1).astype(F32)
    dets[7, 4] = dets[90, 4]                                   # a tied score: the stable sort keeps index order
    got = ops.nms(_dev(dets), 0.6)
    want = R.nms(dets, 0.6, inclusive=False)
    assert got.dtype == torch.long and got.is_cuda and np.array_equal(got.cpu().numpy(), want) and 1 < len(want) < n


def test_roi_pool_autograd(hip_lib):
    rng = np.random.RandomState(42)
    feat = rng.randn(2, 4, 9, 11).astype(F32)
    rois = np.array([[0, 0, 0, 160, 128], [1, 16, 16, 100, 90], [1, 40, 8, 120, 70], [0, 30, 30, 60, 60]], dtype=F32)
    weight = rng.randint(-3, 4, (4, 4, 7, 7)).astype(F32)      # integer-valued: the gradient sums are exact
    x, r = _dev(feat).requires_grad_(), _dev(rois).requires_grad_()
    for layer in (ops.RoIPoolFunction(7, 7, 1.0 / 16), ops.RoIPool(7, 7, 1.0 / 16)):
        x.grad = None
        out = layer(x, r)
        want, arg = R.roi_pool(feat, rois, 1.0 / 16, 7, 7)
        assert np.array_equal(out.detach().cpu().numpy(), want)
        (out * _dev(weight)).sum().backward()
        g_want, terms, _ = R.roi_pool_bwd(weight, rois, arg, feat.shape)
        assert r.grad is None and terms.max() > 1 and np.array_equal(x.grad.cpu().numpy(), g_want.astype(F32))
    assert ops.RoIPoolFunction(7, 7, 1.0 / 16)(_dev(feat), _dev(rois)).requires_grad is False


def test_crop_and_resize_autograd(hip_lib):
    rng = np.random.RandomState(43)
    image = rng.randn(2, 3, 6, 8).astype(F32)
    boxes = np.array([[0, 0, 1, 1], [1, 1, 0, 0], [0.5, 0, 1, 2], [-0.5, -1, 0.5, 1]], dtype=F32)     # lerps are multiples of 1/4
    ind = np.array([0, 1, 1, 0], dtype=np.int32)
    weight = rng.randint(-3, 4, (4, 3, 3, 5)).astype(F32)
    x, b = _dev(image).requires_grad_(), _dev(boxes).requires_grad_()
    for layer in (ops.CropAndResizeFunction(3, 5), ops.CropAndResize(3, 5, 0)):
        x.grad = None
        out = layer(x, b, _dev(ind))
        assert np.array_equal(out.detach().cpu().numpy(), R.crop_and_resize(image, boxes, ind, 3, 5))
        (out * _dev(weight)).sum().backward()
        g_want, terms, _ = R.crop_and_resize_bwd(weight, boxes, ind, image.shape)
        assert b.grad is None and terms.max() > 4 and np.array_equal(x.grad.cpu().numpy(), g_want.astype(F32))
    # the NCHW drop-in of _crop_pool_layer differentiates through the crop and torch's max-pool
    rois = _dev(np.array([[0, 10, 20, 90, 70], [1, 0, 0, 112, 80]], dtype=F32))
    x.grad = None
    proposal.crop_pool_layer(x, rois, max_pool=True).sum().backward()
    assert x.grad is not None and x.grad.abs().sum().item() > 0


def test_roi_crop_nhwc_output_is_a_conv_input(hip_lib):
    """[R,7,7,C] fp16 from ft_roi_crop_nhwc_fwd goes into ft_conv2d_fwd as N = R, Hi = Wi = 7 with a 1x1 identity weight: the
    products are x * 1 and x * 0, the fp32 sums are exact, so the conv returns its input bit for bit iff the layout is the one it reads."""
    C, Rn = 64, 5
    rng = np.random.RandomState(44)
    feat = _dev(rng.randn(1, 6, 9, C).astype(F32)).half()
    rois = _dev(np.concatenate((np.zeros((Rn, 1)), rng.uniform(0, 60, (Rn, 2)), rng.uniform(70, 140, (Rn, 2))), 1).astype(F32))
    x = proposal.roi_crop_nhwc(feat, rois)
    assert x.shape == (Rn, 7, 7, C) and x.abs().sum().item() > 0
    d = ConvDesc()
    d.dtype, d.N, d.Hi, d.Wi, d.Cin, d.x_cstride, d.x_coff = FT_F16, Rn, 7, 7, C, C, 0
    d.Cout, d.kh, d.kw, d.stride, d.pad, d.transposed, d.Ho, d.Wo = C, 1, 1, 1, 0, 0, 7, 7
    d.y_cstride, d.y_coff, d.out_layout = C, 0, FT_LAYOUT_NHWC
    w, _ = pack_conv_weights(torch.eye(C).reshape(C, C, 1, 1), d, dtype=torch.float16, device=x.device)
    y = torch.full_like(x, 7.0)
    torch.cuda.synchronize()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(hip_lib.ft_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), None, None, None, y.data_ptr(), stream), "ft_conv2d_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), x.view(torch.int16))


def test_python_wrappers_refuse_fp16_and_wrong_shapes_on_the_device(hip_lib):
    dev = torch.device("cuda:0")
    feat, rois = torch.zeros(1, 8, 4, 4, device=dev), torch.zeros(2, 5, device=dev)
    boxes, ind = torch.zeros(2, 4, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.RoIPoolFunction(7, 7, 1 / 16)(feat.half(), rois)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.CropAndResizeFunction(7, 7)(feat.half(), boxes, ind)
    with pytest.raises(FlowtrackHipError, match="fp32 CUDA"):
        ops.nms(torch.zeros(4, 5, device=dev).half(), 0.7)
    with pytest.raises(FlowtrackHipError, match="shape"):
        ops.RoIPoolFunction(7, 7, 1 / 16)(feat, rois[:, :4])
    with pytest.raises(FlowtrackHipError, match="shape"):
        ops.CropAndResizeFunction(7, 7)(feat, rois, ind)
    with pytest.raises(FlowtrackHipError, match="int32"):
        ops.CropAndResizeFunction(7, 7)(feat, boxes, ind.long())
    with pytest.raises(FlowtrackHipError, match="int32"):
        ops.CropAndResizeFunction(7, 7)(feat, boxes, ind[:1])
    with pytest.raises(FlowtrackHipError, match="invalid argument"):
        proposal.roi_crop_nhwc(torch.zeros(1, 4, 4, 12, device=dev), rois)          # C % 8: the entry's refusal surfaces
    with pytest.raises(FlowtrackHipError, match="invalid argument"):
        proposal.roi_crop_nhwc(torch.zeros(1, 1, 4, 8, device=dev), rois)           # H < 2
    with pytest.raises(FlowtrackHipError, match="16384"):
        ops.box_nms_sorted(torch.zeros(16385, 5, device=dev), 0.7)
    assert ops.nms(torch.zeros(0, 5, device=dev), 0.7).shape == (0,)
    assert ops.RoIPoolFunction(7, 7, 1 / 16)(feat, rois[:0]).shape == (0, 8, 7, 7)
    assert proposal.roi_crop_nhwc(torch.zeros(1, 4, 4, 8, device=dev), rois[:0]).shape == (0, 7, 7, 8)
