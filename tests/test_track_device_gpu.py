"""The device tracking pass on the GPU (csrc/track_ops.hip through the C ABI, tracking/device_pass.py): every comparison is
bit-exact (np.array_equal, float values included) against the host functions the kernels restate — propagate_keypoints,
box_propagation, nms, boxes_to_center_scale, heatmap_rows_to_image and the lines of tools/tracking/demo.tracking_pass_steps
around them (tests/track_device_ref.py only arranges their calls)."""
import numpy as np
import pytest
import torch

from flowtrack.pytorch_amd import _lib

import track_device_ref as R

pytestmark = pytest.mark.gpu
RH, RW = 256, 192


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _sync_ok():
    torch.cuda.synchronize()


# ---- ft_track_propagate ---------------------------------------------------------------------------------------------------
def _poses(P, K, seed):
    """Key points around a 24 x 32 image with the edge cases of the truncate-then-clip rule and of the joint mask."""
    rng = np.random.RandomState(seed)
    kp = np.concatenate((rng.uniform(-4, 36, (P, K, 1)), rng.uniform(-4, 28, (P, K, 1)), rng.uniform(0.1, 1.0, (P, K, 1))), 2)
    kp[0, 0, :2] = (-0.5, -1.5)                          # int(-0.5) = 0, int(-1.5) = -1 -> clipped to 0: truncation, not floor
    kp[0, 1, :2] = (-1.5, -0.5)
    kp[0, 2, :2] = (40.25, 30.75)                        # past both edges
    kp[0, 3, :2] = (31.999, 23.999)
    kp[0, 4, 2] = 0.0                                    # masked joints: score 0 and a negative score
    kp[0, 5, 2] = -0.3
    if P > 3:
        kp[3, :, 2] = 0.0                                # a person with every joint masked
        kp[2, :, :2] += 30.0                             # a person whose joints all lie past the image: min above max(H, W) needs no fill
    return kp.astype(np.float32)


@pytest.mark.parametrize("K", [17, 16])
@pytest.mark.parametrize("P,n_old", [(6, 0), (6, 2), (1, 0), (1, 2)])
def test_propagate_matches_host_functions(hip_lib, P, n_old, K):
    rng = np.random.RandomState(10 * P + n_old + K)
    H, W = 24, 32
    flow = rng.uniform(-6, 6, (2, H, W)).astype(np.float32)
    kp = _poses(P, K, K + P)
    older = rng.uniform(-6, 40, (n_old, P, K, 2))
    if n_old:
        older[0, 0, 0] = (-0.5, -1.5)
        older[1, 0, 1] = (45.5, 1e6)
    want_moved, want_boxes = R.propagate_ref(kp, flow, older)
    d_kp, d_flow, d_old = _dev(kp), _dev(flow), _dev(older) if n_old else None
    moved = torch.full((1 + n_old, P, K, 2), -7.0, dtype=torch.float64, device="cuda")
    boxes = torch.full((P, 4), -7.0, dtype=torch.float32, device="cuda")
    st = hip_lib.ft_track_propagate(_ptr(d_kp), _ptr(d_flow), H, W, _ptr(d_old), n_old, P, K, _ptr(moved), _ptr(boxes), None)
    assert st == _lib.FT_OK
    _sync_ok()
    assert np.array_equal(moved.cpu().numpy(), want_moved)
    assert np.array_equal(boxes.cpu().numpy(), want_boxes)


# ---- ft_track_select ------------------------------------------------------------------------------------------------------
def _boxes(rng, n, span=300.0, size=(20.0, 90.0)):
    xy = rng.uniform(0, span, (n, 2))
    wh = rng.uniform(size[0], size[1], (n, 2))
    return np.concatenate((xy, xy + wh, rng.uniform(0.05, 1.0, (n, 1))), 1).astype(np.float32)


def _run_select(lib, dets, kp_det, prop, prev, M, K, thresh, max_keep, cap, bucket, null_count=False):
    n, P = len(dets), len(prop)
    d_dets, d_kp = (_dev(dets), _dev(kp_det)) if n else (None, None)
    d_prop, d_prev = (_dev(prop), _dev(prev)) if P else (None, None)
    d_m = None if null_count else _dev(np.array([M], np.int32))
    out = {"boxes": torch.full((cap, 5), -7.0, device="cuda"), "src": torch.full((cap,), -7, dtype=torch.int32, device="cuda"),
           "count": torch.full((1,), -7, dtype=torch.int32, device="cuda"), "kps": torch.full((cap, K, 3), -7.0, device="cuda"),
           "nprop": torch.full((1,), -7, dtype=torch.int32, device="cuda"),
           "prop_slot": torch.full((bucket,), -7, dtype=torch.int32, device="cuda"), "params": torch.full((bucket, 3), -7.0, device="cuda")}
    st = lib.ft_track_select(_ptr(d_dets), _ptr(d_kp), n, _ptr(d_prop), _ptr(d_prev), P, _ptr(d_m), K, thresh, max_keep, cap, RH, RW, bucket,
                             *[_ptr(out[k]) for k in ("boxes", "src", "count", "kps", "nprop", "prop_slot", "params")], None)
    if st != _lib.FT_OK:
        return st, None
    _sync_ok()
    return st, {k: v.cpu().numpy() for k, v in out.items()}


def _check_select(lib, dets, prop, prev, M, thresh, max_keep, cap, bucket, K=17, seed=0, null_count=False):
    kp_det = np.random.RandomState(seed).uniform(0, 300, (len(dets), K, 3)).astype(np.float32)
    st, got = _run_select(lib, dets, kp_det, prop, prev, M, K, thresh, max_keep, cap, bucket, null_count)
    assert st == _lib.FT_OK
    want = R.select_ref(dets, kp_det, prop, prev, M, np.float32(thresh), max_keep, RH, RW, bucket, K)
    c, m = want["count"], want["nprop"]
    assert int(got["count"][0]) == c and int(got["nprop"][0]) == m
    assert np.array_equal(got["src"][:c], want["src"]) and (got["src"][c:] == -1).all()
    assert np.array_equal(got["boxes"][:c], want["boxes"]) and not got["boxes"][c:].any()
    assert np.array_equal(got["kps"][:c], want["kps"]) and not got["kps"][c:].any()
    assert np.array_equal(got["prop_slot"][:m], want["prop_slot"]) and (got["prop_slot"][m:] == -1).all()
    assert np.array_equal(got["params"], want["params"])
    return want


def _prev(rng, P):
    """The previous frame's boxes [P,5]: only their scores are read."""
    return np.concatenate((np.zeros((P, 4)), rng.uniform(0.05, 1.0, (P, 1))), 1).astype(np.float32)


def test_select_passes_detector_boxes_through_without_previous_poses(hip_lib):
    rng = np.random.RandomState(1)
    dets = _boxes(rng, 5)
    dets[1] = dets[0]                                    # duplicates stay: no NMS on this path
    for null_count in (False, True):
        want = _check_select(hip_lib, dets, _boxes(rng, 3)[:, :4], _prev(rng, 3), 0, 0.3, 2, 6, 4, null_count=null_count)
        assert want["count"] == 5 and want["nprop"] == 0  # max_keep = 2 does not cut either


def test_select_without_detector_boxes(hip_lib):
    rng = np.random.RandomState(2)
    want = _check_select(hip_lib, np.zeros((0, 5), np.float32), _boxes(rng, 3, span=400.0)[:, :4], _prev(rng, 3), 3, 0.3, 4, 4, 4)
    assert want["nprop"] == want["count"] >= 1


def test_select_is_stable_on_equal_scores(hip_lib):
    rng = np.random.RandomState(3)
    dets, prop, prev = _boxes(rng, 9, span=150.0), _boxes(rng, 7, span=150.0)[:, :4], _prev(rng, 7)
    dets[:, 4] = 0.5
    prev[:, 4] = 0.5
    prev[2, 4] = dets[4, 4] = 0.75                       # two groups of ties, each across the detector / propagated boundary
    _check_select(hip_lib, dets, prop, prev, 7, 0.3, 16, 16, 8, seed=3)
    _check_select(hip_lib, dets, prop, prev, 5, 0.3, 16, 16, 8, seed=3)    # M < P: the last two propagated boxes are not in the union


def test_select_suppresses_at_the_threshold_and_keeps_a_zero_area_pair(hip_lib):
    a = np.array([[10, 20, 60, 120, 0.9], [200, 20, 260, 120, 0.8]], np.float32)
    prop, prev = a[:1, :4].copy(), np.array([[0, 0, 0, 0, 0.7]], np.float32)
    want = _check_select(hip_lib, a, prop, prev, 1, 1.0, 4, 4, 4)           # identical boxes: IoU = 1.0 >= 1.0 suppresses
    assert want["count"] == 2 and want["nprop"] == 0
    # zero-area pair: x2 = x1 - 1 makes the +1 width 0, IoU = 0 / 0 = NaN, which is not >= thresh: both stay
    z = np.array([[50, 50, 49, 80, 0.9]], np.float32)
    want = _check_select(hip_lib, z, z[:, :4].copy(), np.array([[0, 0, 0, 0, 0.6]], np.float32), 1, 0.3, 4, 4, 4)
    assert want["count"] == 2 and want["nprop"] == 1


def test_select_max_keep_cuts_the_kept_list(hip_lib):
    rng = np.random.RandomState(4)
    dets, prop, prev = _boxes(rng, 6, span=600.0, size=(10, 30)), _boxes(rng, 6, span=600.0, size=(10, 30))[:, :4], _prev(rng, 6)
    want = _check_select(hip_lib, dets, prop, prev, 6, 0.3, 5, 8, 8, seed=4)
    assert want["count"] == 5
    want = _check_select(hip_lib, dets, prop, prev, 6, 0.3, 1, 8, 8, seed=4)
    assert want["count"] == 1


def test_select_every_kept_box_from_the_detector(hip_lib):
    rng = np.random.RandomState(5)
    dets = _boxes(rng, 5, span=30.0, size=(40, 60))
    dets[:, [0, 2]] += np.arange(5, dtype=np.float32)[:, None] * 110    # side by side: no detector box touches another
    dets[:, 4] = rng.uniform(0.6, 1.0, 5)
    prop = dets[:, :4] + np.float32(1.0)                 # each propagated box sits on a detector box that out-scores it
    want = _check_select(hip_lib, dets, prop, _prev(rng, 5) * np.float32(0.5), 5, 0.3, 10, 10, 8, seed=5)
    assert want["nprop"] == 0 and want["count"] == 5 and (want["params"] == (0, 0, 1)).all()


@pytest.mark.parametrize("K", [17, 16])
def test_select_300_box_union(hip_lib, K):
    rng = np.random.RandomState(6)
    dets, prop, prev = _boxes(rng, 150, span=500.0), _boxes(rng, 150, span=500.0)[:, :4], _prev(rng, 150)
    want = _check_select(hip_lib, dets, prop, prev, 150, 0.3, 300, 300, 256, K=K, seed=6)     # five 64-bit mask words
    assert 64 < want["count"] < 300 and 0 < want["nprop"] < want["count"]
    _check_select(hip_lib, dets, prop, prev, 150, 0.5, 100, 300, 256, K=K, seed=6)


def test_select_refuses_what_it_cannot_run(hip_lib):
    rng = np.random.RandomState(7)
    big, prev = _boxes(rng, 300), _prev(rng, 300)
    kp = np.zeros((300, 17, 3), np.float32)
    st, _ = _run_select(hip_lib, big, kp, big[:213, :4], prev[:213], 213, 17, 0.3, 600, 600, 256)         # n + P = 513
    assert st == _lib.FT_ERR_UNSUPPORTED
    st, _ = _run_select(hip_lib, big[:4], np.zeros((4, 33, 3), np.float32), big[:4, :4], prev[:4], 4, 33, 0.3, 8, 8, 4)   # K = 33
    assert st == _lib.FT_ERR_UNSUPPORTED
    st, _ = _run_select(hip_lib, big[:4], kp[:4], big[:6, :4], prev[:6], 6, 17, 0.3, 8, 8, 4)             # bucket 4 < min(cap 8, P 6)
    assert st == _lib.FT_ERR_UNSUPPORTED
    st, _ = _run_select(hip_lib, big[:9], kp[:9], big[:2, :4], prev[:2], 2, 17, 0.3, 8, 8, 4)             # n = 9 > cap = 8
    assert st == _lib.FT_ERR_INVALID_ARG


# ---- ft_track_place_rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hm_hw", [(64, 48), (96, 72)])
@pytest.mark.parametrize("nprop", [0, 1, 5])
def test_place_rows_matches_heatmap_rows_to_image(hip_lib, hm_hw, nprop):
    rng = np.random.RandomState(8 + nprop)
    K, bucket, cap = 17, 8, 10
    h, w = hm_hw
    boxes = _boxes(rng, cap, span=400.0, size=(15.0, 200.0))
    rows = np.concatenate((np.round(rng.uniform(0, w - 1, (bucket, K, 1)) * 4) / 4, np.round(rng.uniform(0, h - 1, (bucket, K, 1)) * 4) / 4,
                           rng.uniform(0, 1, (bucket, K, 1))), 2).astype(np.float32)
    slots = rng.permutation(cap)[:nprop].astype(np.int32)
    kps = rng.uniform(0, 300, (cap, K, 3)).astype(np.float32)              # the detector rows already there must stay
    slot_buf = np.full((bucket,), -1, np.int32)
    slot_buf[:nprop] = slots
    d_kps, d_rows, d_boxes, d_slots, d_n = _dev(kps), _dev(rows), _dev(boxes), _dev(slot_buf), _dev(np.array([nprop], np.int32))
    st = hip_lib.ft_track_place_rows(_ptr(d_rows), _ptr(d_boxes), _ptr(d_slots), _ptr(d_n), bucket, cap, K, h, w, RH, RW, _ptr(d_kps), None)
    assert st == _lib.FT_OK
    _sync_ok()
    assert np.array_equal(d_kps.cpu().numpy(), R.place_rows_ref(kps, rows, boxes, slots, (h, w), RH, RW))


# ---- the whole pass against the host pass ---------------------------------------------------------------------------------
def test_device_pass_replays_as_the_host_pass(hip_lib):
    """DeviceTrackingPass.run on a 6-frame clip, then the host tracking_pass on the same detector key points and flows, its
    pose_boxes answering with the rows the device pass placed (the network's own numerics cancel out): the host pass must ask
    for exactly the device pass's propagated boxes and end with the same boxes, key points and ids."""
    import types
    from flowtrack.pytorch_amd.tracking import DeviceTrackingPass, PoseRunner
    from tools.tracking import demo
    dev = torch.device("cuda:0")
    args = types.SimpleNamespace(pose_backbone=50, pose_model="", flow_net="FlowNet2S", flow_model="", fp16=True)
    pose_net, flow_net = demo.build_nets(args, dev)
    frames, dets = demo.synthetic_clip(6, H=192, W=256, n_people=3, seed=4)
    runner = PoseRunner(pose_net)
    fr, flows, kp_all, _ = demo._batched_phases(frames, dets, pose_net, flow_net, 0, 1, 16, 6, None, flow_net, dev, runner, on_device=True)
    runner.close()
    dpass = DeviceTrackingPass(pose_net)
    got = dpass.run(fr, dets, kp_all, flows, 0.3, "2x")
    dpass.close()
    asked = []

    def pose_boxes(t, boxes):
        prop = got[t]["src"] >= len(dets[t])
        assert np.array_equal(np.asarray(boxes, np.float32), got[t]["boxes"][prop, :4])
        asked.append(t)
        return got[t]["keypoints"][prop]

    kp_host = kp_all.cpu().numpy()
    want = demo.tracking_pass(dets, [kp_host[t, :len(dets[t])] for t in range(6)], flows.cpu().numpy(), pose_boxes, 0.3, "2x")
    assert len(got) == len(want) == 6 and asked, "no propagated box survived in any frame: the replay checked nothing"
    for g, w in zip(got, want):
        assert np.array_equal(g["boxes"], w["boxes"]) and np.array_equal(g["keypoints"], w["keypoints"]) and list(g["ids"]) == list(w["ids"])
