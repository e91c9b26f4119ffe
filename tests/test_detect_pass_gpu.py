"""The detector's clip pass on the GPU against the per-frame path it restates: proposal.proposal_layer_device against
proposal.proposal_layer on the same plan outputs, detection.test.detect_persons_clip against detect_persons frame by frame (both
trunks, both dtypes, with and without extra boxes), no device -> host transfer inside clip_enqueue, and the tracking tool with
--detector.  Every comparison is bit for bit: both paths replay the same two plans and run the same kernels around them; what
differs is the sort (ft_topk_desc_f32 for torch.sort), the blob (ft_proposal_rois_fwd) and the person NMS (ft_detect_select_fwd)."""
import functools

import numpy as np
import pytest
import torch

from conftest import ROOT
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.detection import nets, proposal, test as det_test

pytestmark = pytest.mark.gpu
SEED, TARGET, MAX_SIZE = 7, 75, 125                    # 50 x 72 frames -> 75 x 108 blobs, as tests/test_detect_net_gpu.py
K, PERSON, A, POST = 3, 1, 9, 32
DTYPES = {"fp32": torch.float32, "fp16": torch.float16}
TRUNKS = ("resnetv1", "vgg16")


@functools.lru_cache(maxsize=None)
def _state_dict(trunk):
    net = nets.vgg16() if trunk == "vgg16" else nets.resnetv1(50)
    net.create_architecture(K, tag="default")
    fill = synth.fill_vgg_detector_state_dict if trunk == "vgg16" else synth.fill_detector_state_dict
    return fill(net.state_dict(), SEED)


@functools.lru_cache(maxsize=None)
def _net(trunk, dtype_id):
    net = nets.vgg16() if trunk == "vgg16" else nets.resnetv1(50)
    net.create_architecture(K, tag="default")
    net.load_state_dict(_state_dict(trunk))
    net = net.cuda().eval()
    net.compute_dtype = DTYPES[dtype_id]
    net.rpn_post_nms_topN = POST
    return net


@functools.lru_cache(maxsize=None)
def _frames():
    return np.stack([synth.detector_frame(SEED + t, 50, 72) for t in range(3)])


def _extras():
    """Per-frame extra boxes of different lengths (one frame has none): scores that tie with each other and sit among the detector's."""
    a = np.array([[5, 5, 30, 40, 0.99], [4, 6, 31, 41, 0.5], [40, 10, 60, 45, 0.2], [41, 11, 61, 46, 0.2]], dtype=np.float32)
    return [a, None, a[1:3]]


@pytest.mark.parametrize("trunk", TRUNKS)
@pytest.mark.parametrize("dtype_id", sorted(DTYPES))
def test_proposal_layer_device_is_proposal_layer(hip_lib, trunk, dtype_id):
    net = _net(trunk, dtype_id)
    plan, im_info, _, _ = det_test.stage_frame(net, _frames()[0], TARGET, MAX_SIZE)
    net.run(plan)
    info = [float(v) for v in im_info]
    blob, _ = proposal.proposal_layer(plan.rpn_cls_prob, plan.rpn_bbox_pred, info, "TEST", 16, plan.anchors, A, post_nms_topN=POST)
    n = int(blob.shape[0])
    assert 0 < n <= POST
    for rows in (POST, n + 3 if n + 3 != POST else n + 4, max(n - 1, 1)):          # the plan's row count, another one, fewer rows than kept
        rois = torch.full((rows, 5), 3.0, dtype=torch.float32, device="cuda")        # stale contents
        out, n_rois = proposal.proposal_layer_device(plan.rpn_cls_prob, plan.rpn_bbox_pred, info, "TEST", 16, plan.anchors, A, rois,
                                                     post_nms_topN=POST)
        assert out is rois and n_rois.dtype == torch.int32 and n_rois.is_cuda
        m = min(n, rows)
        assert int(n_rois.item()) == m
        assert torch.equal(rois[:m].view(torch.int32), blob[:m].contiguous().view(torch.int32)) and not rois[m:].any()


@pytest.mark.parametrize("with_extras", [False, True], ids=["plain", "prop_dets"])
@pytest.mark.parametrize("trunk", TRUNKS)
@pytest.mark.parametrize("dtype_id", sorted(DTYPES))
def test_clip_is_detect_persons_per_frame(hip_lib, dtype_id, trunk, with_extras):
    net = _net(trunk, dtype_id)
    frames = _frames()
    extras = _extras() if with_extras else None
    want = [det_test.detect_persons(net, frames[t], PERSON, 0.3, None if extras is None else extras[t], target_size=TARGET, max_size=MAX_SIZE)
            for t in range(len(frames))]
    assert all(len(w) >= 1 for w in want) and not np.array_equal(want[0], want[1])
    plans = len(net._plans)
    for call in range(2):                                                            # the second call replays the same plans
        got = det_test.detect_persons_clip(net, frames, PERSON, 0.3, 0.0, extras, target_size=TARGET, max_size=MAX_SIZE)
        assert len(got) == len(want) and len(net._plans) == plans
        for t, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.float32 and g.shape == w.shape, (call, t, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (call, t)
    plan = next(iter(net._plans.values()))
    assert list(plan.heads) == [POST]                                                # one head plan: both paths replay it
    # frames already on the device, extras as a [T,M,5] tensor: the same results
    if with_extras:
        dense = np.zeros((3, 4, 5), dtype=np.float32)
        dense[:] = _extras()[0]
        got = det_test.detect_persons_clip(net, torch.from_numpy(frames).cuda(), PERSON, 0.3, 0.0, torch.from_numpy(dense).cuda(),
                                           target_size=TARGET, max_size=MAX_SIZE)
        for t in range(3):
            w = det_test.detect_persons(net, frames[t], PERSON, 0.3, dense[t], target_size=TARGET, max_size=MAX_SIZE)
            assert np.array_equal(got[t].view(np.uint32), w.view(np.uint32)), t


def test_clip_screen_and_cap(hip_lib):
    net = _net("resnetv1", "fp32")
    frames = _frames()
    full = det_test.detect_persons_clip(net, frames, PERSON, 0.3, target_size=TARGET, max_size=MAX_SIZE)
    capped = det_test.detect_persons_clip(net, frames, PERSON, 0.3, target_size=TARGET, max_size=MAX_SIZE, cap=2)
    assert all(np.array_equal(c, f[:2]) for c, f in zip(capped, full))
    none = det_test.detect_persons_clip(net, frames, PERSON, 0.3, min_score=2.0, target_size=TARGET, max_size=MAX_SIZE)
    assert all(d.shape == (0, 5) for d in none)
    assert det_test.detect_persons_clip(net, frames[:0], PERSON, target_size=TARGET, max_size=MAX_SIZE) == []


def _sync_debug_mode_works():
    """Whether this torch build reports synchronising calls in the "error" mode (it is a CUDA feature that a ROCm build may leave out)."""
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_clip_enqueue_makes_no_device_to_host_transfer(hip_lib):
    net = _net("resnetv1", "fp16")
    frames = torch.from_numpy(_frames()).cuda()
    extras = torch.from_numpy(np.tile(_extras()[0], (3, 1, 1))).cuda()
    want = det_test.detect_persons_clip(net, frames, PERSON, 0.3, 0.0, extras, target_size=TARGET, max_size=MAX_SIZE)      # plans built
    if not _sync_debug_mode_works():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not report a synchronising call on this torch build")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        handle = det_test.clip_enqueue(net, frames, PERSON, 0.3, 0.0, extras, target_size=TARGET, max_size=MAX_SIZE)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = det_test.clip_finish(handle)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_tracking_demo_with_detector(hip_lib, capsys):
    import sys
    sys.path.insert(0, ROOT)
    from tools.tracking import demo
    argv = ["--frames", "4", "--height", "192", "--width", "256", "--people", "3", "--fp16", "--detector", "res50", "--det_classes", "3",
            "--det_person_id", "1", "--det_target_size", "75", "--det_max_size", "125"]
    args = demo.build_parser().parse_args(argv)
    out, dets, tm = demo.run(args)
    line = capsys.readouterr().out
    assert "detector res50" in line and "track ids" in line and tm["detect_s"] > 0
    assert len(out) == 4 and all(len(f["boxes"]) == len(f["keypoints"]) == len(f["ids"]) for f in out) and any(len(f["ids"]) for f in out)
    frames, gen_dets = demo.synthetic_clip(4, 192, 256, n_people=3)
    det_net = demo.build_detector(args, torch.device("cuda", 0))
    assert len(dets) == 4
    for t in range(4):
        want = det_test.detect_persons(det_net, frames[t], 1, 0.3, target_size=75, max_size=125)
        assert dets[t].dtype == np.float32 and dets[t].shape[1] == 5
        assert np.array_equal(dets[t], want) and not np.array_equal(dets[t], gen_dets[t])
    assert np.array_equal(out[0]["boxes"], dets[0])    # frame 0 has nothing propagated: the detector's boxes pass through
