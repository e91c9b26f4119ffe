"""Host side of the device tracking pass (tracking/device_pass.py), no GPU: the ids HistoryTracker assigns from a moved-pose
history are FlowTracker's, and DeviceTrackingPass refuses what it cannot run before it touches a device."""
import numpy as np
import pytest

from flowtrack.pytorch_amd.tracking import DeviceTrackingPass, FlowTracker, HistoryTracker

import track_device_ref as R

K, H, W, T = 17, 96, 128, 8


def _clip(seed):
    """8 frames of 2-5 people (K = 17) walking with the flow, in a shuffled order per frame: two leading frames without
    detections, people who leave for ONE frame (their track ages and is propagated twice before it is matched again), one who
    leaves for two.  Returns (kps per frame [n_t,K,3], boxes per frame [n_t,5], flows [T-1,2,H,W], person index per row)."""
    rng = np.random.RandomState(seed)
    people = 5
    vel = np.array([2.5, -1.5]) if seed % 2 else np.array([-2.0, 1.0])
    base = np.stack((rng.uniform(25, W - 45, people), rng.uniform(30, H - 40, people)), 1)
    shape = rng.uniform(-12, 12, (people, K, 2))
    score = rng.uniform(0.3, 0.95, (people, K))
    score[1, 3] = 0.0                                                        # a joint the OKS does not count
    present = np.ones((T, people), dtype=bool)
    present[:2] = False                                                      # two leading frames without detections
    present[4, 0] = present[5, 2] = False                                    # gone for one frame
    present[5:7, 3] = False                                                  # gone for two frames (matched again only with max_age 2)
    present[:, 4] = rng.uniform(size=T) > 0.5                                # 2 to 5 people per frame
    present[:2, 4] = False
    flows = (vel[None, :, None, None] + rng.uniform(-0.4, 0.4, (T - 1, 2, H, W))).astype(np.float32)
    kps, boxes, who = [], [], []
    for t in range(T):
        idx = rng.permutation(np.nonzero(present[t])[0])
        xy = base[idx, None, :] + shape[idx] + vel * t + rng.uniform(-0.3, 0.3, (len(idx), K, 2))
        kp = np.concatenate((xy, score[idx][..., None]), 2).astype(np.float32)
        bx = np.concatenate((xy.min(1) - 4, xy.max(1) + 4, rng.uniform(0.5, 1.0, (len(idx), 1))), 1).astype(np.float32)
        kps.append(kp.reshape(-1, K, 3))
        boxes.append(bx.reshape(-1, 5))
        who.append(idx)
    return kps, boxes, flows, who


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("max_age", [1, 2])
def test_history_tracker_assigns_flow_tracker_ids(seed, max_age):
    kps, boxes, flows, who = _clip(seed)
    assert [len(k) for k in kps[:2]] == [0, 0] and all(2 <= len(k) <= 5 for k in kps[2:])
    hist = R.history_from_flows(kps, flows, max_age, cap=6)
    ref, got = FlowTracker(max_age=max_age), HistoryTracker(max_age=max_age)
    ids_ref, ids_got = [], []
    for t in range(T):
        has_flow = t > 0 and len(kps[t - 1]) > 0                             # tracking_pass_steps: flow only behind a frame with poses
        ids_ref.append(ref.update(kps[t], boxes[t], flows[t - 1] if has_flow else None))
        ids_got.append(got.update(kps[t], boxes[t], hist[t] if has_flow else None))
    assert ids_got == ids_ref
    assert got.next_id == ref.next_id and sorted(got.tracks) == sorted(ref.tracks)
    for tid in ref.tracks:                                                   # the tracks themselves, aged ones included, bit for bit
        assert np.array_equal(got.tracks[tid]["kpts"], ref.tracks[tid]["kpts"]) and got.tracks[tid]["age"] == ref.tracks[tid]["age"]
    # the clip does what it was built for: a person who was away for one frame comes back under the id they had (so the match
    # went through a pose propagated twice), the one away for two frames only with max_age = 2
    by_person = lambda t, p: ids_ref[t][list(who[t]).index(p)]               # noqa: E731
    assert by_person(5, 0) == by_person(3, 0) and by_person(6, 2) == by_person(4, 2)
    assert (by_person(7, 3) == by_person(4, 3)) == (max_age == 2)


def test_history_step_without_flow_ages_unmoved():
    rng = np.random.RandomState(5)
    prev = rng.uniform(0, 50, (3, 4, K, 2))
    cur = R.history_step(prev, np.zeros((0, K, 3)), None)
    assert np.array_equal(cur[1:], prev[:-1]) and not cur[0].any()


def test_device_pass_refuses_before_touching_a_device():
    dp = DeviceTrackingPass(pose_net=object())                               # no network, no GPU: nothing may be reached
    dets = [np.zeros((3, 5), np.float32), np.zeros((5, 5), np.float32)]
    with pytest.raises(ValueError, match="max_boxes"):
        dp.run(None, dets, None, None, max_boxes=None)
    with pytest.raises(ValueError, match="exceed the cap"):
        dp.run(None, dets, None, None, max_boxes=4)                          # frame 1 has 5 detector boxes
    with pytest.raises(ValueError, match="device NMS"):
        dp.run(None, [np.zeros((200, 5), np.float32), np.zeros((200, 5), np.float32)], None, None, max_boxes=400)
    sched = dp.schedule([np.zeros((0, 5)), np.zeros((3, 5)), np.zeros((1, 5)), np.zeros((9, 5))], "2x")
    assert [(f["n"], f["cap"], f["prev_cap"], f["bucket"], f["has_prev"]) for f in sched] == \
        [(0, 4, 0, 4, False), (3, 6, 4, 4, False), (1, 4, 6, 4, True), (9, 18, 4, 4, True)]
    assert dp.schedule([np.zeros((9, 5)), np.zeros((9, 5))], "2x")[1]["bucket"] == 32
