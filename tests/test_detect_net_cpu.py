"""The detector network without a GPU: tests/detect_net_ref.py against every tensor the reference recorded
(tests/golden/detect_net_golden.npz), the state_dict contract of detection.nets.resnetv1, and the derived error bounds of the four
glue kernels against float32 numpy runs of their own references."""
import functools
import os

import numpy as np
import pytest
import torch

import detect_net_ref as R
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from flowtrack.pytorch_amd.detection import nets, test as det_test

G = np.load(os.path.join(GOLDEN, "detect_net_golden.npz"), allow_pickle=False)
SEED, TARGET, MAX_SIZE = int(G["seed"]), int(G["target_size"]), int(G["max_size"])
K, PERSON = int(G["num_classes"]), int(G["person_id"])
CASES = ("a", "b")
CONTINUOUS = ("blob", "net_conv", "rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "rois", "cls_score", "cls_prob", "bbox_pred", "scores",
              "pred_boxes")


@functools.lru_cache(maxsize=None)
def _net(depth=50):
    net = nets.resnetv1(depth)
    net.create_architecture(K, tag="default")
    return net


@functools.lru_cache(maxsize=None)
def _state_dict():
    return synth.fill_detector_state_dict(_net().state_dict(), SEED)


def _frame(case):
    h, w = (int(v) for v in G[case + "_frame_hw"])
    return synth.detector_frame(SEED, h, w)


@functools.lru_cache(maxsize=None)
def _restated(case):
    return R.im_detect(_state_dict(), _frame(case), 50, TARGET, MAX_SIZE)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    mine = _restated(case)
    for k in CONTINUOUS:
        want = G[f"{case}_{k}"]
        assert np.shape(mine[k]) == want.shape, k
        err = float(np.abs(np.asarray(mine[k], dtype=np.float64) - want.astype(np.float64)).max())
        print(f"case {case} {k}: max abs {err:.2e} (max |golden| {np.abs(want).max():.3g})")
        assert err <= 1e-5, (k, err)
    assert np.array_equal(mine["im_info"], G[case + "_im_info"])
    persons = R.detect_persons(mine["scores"], mine["pred_boxes"], PERSON, 0.3)
    assert persons.shape == G[case + "_persons"].shape and np.abs(persons - G[case + "_persons"]).max() <= 1e-5


@pytest.mark.parametrize("case", CASES)
def test_golden_is_not_degenerate(case):
    """The conditions the golden's seed was searched for, on the stored tensors."""
    A = G[case + "_rpn_cls_prob"].shape[-1] // 2
    fg, pp = G[case + "_rpn_cls_prob"][..., A:], G[case + "_cls_prob"][:, PERSON]
    assert np.abs(G[case + "_net_conv"]).max() <= 32
    assert ((fg > 0.1) & (fg < 0.9)).mean() >= 0.25 and ((pp > 0.1) & (pp < 0.9)).mean() >= 0.25
    assert np.abs(G[case + "_rpn_bbox_pred"]).max() <= 1 and np.abs(G[case + "_bbox_pred"]).max() <= 1
    assert 8 <= len(G[case + "_rois"]) < fg.size
    assert 2 <= len(G[case + "_persons"]) < len(G[case + "_rois"])


@pytest.mark.parametrize("depth", (50, 101))
def test_state_dict_keys_and_shapes(depth):
    sd = _net(depth).state_dict()
    keys, shapes = [str(k) for k in G[f"keys_{depth}"]], [str(s) for s in G[f"shapes_{depth}"]]
    assert list(sd) == keys
    assert [";".join(str(d) for d in sd[k].shape) for k in keys] == shapes
    if depth == 50:
        assert len(keys) == 328 and not any(k.startswith("resnet.fc.") for k in keys)


def test_load_state_dict_rule():
    net = nets.resnetv1(50)
    net.create_architecture(K, tag="default")
    sd = dict(_state_dict())
    sd["resnet.fc.weight"], sd["resnet.fc.bias"] = torch.zeros(1000, 2048), torch.zeros(1000)      # an old checkpoint
    net.load_state_dict(sd)
    got = net.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in got)
    del sd["rpn_net.bias"]
    with pytest.raises(KeyError):
        net.load_state_dict(sd)
    trunk = nets.resnetv1(50)
    trunk.create_architecture(K, tag="default")
    trunk.load_pretrained_cnn({k[len("resnet."):]: v for k, v in _state_dict().items() if k.startswith("resnet.")})
    assert torch.equal(trunk.state_dict()["resnet.layer3.5.conv3.weight"], _state_dict()["resnet.layer3.5.conv3.weight"])


def test_init_statistics():
    """nets/network.py:393-409: N(0, 0.01) head layers, N(0, 0.001) for bbox_pred_net, zero biases.  The sample std of n values
    is within 5 / sqrt(2 n) of the true one far beyond any seed's luck."""
    torch.manual_seed(0)
    net = nets.resnetv1(101)
    net.create_architecture(81, tag="default")
    for name, std in (("rpn_net", 0.01), ("rpn_cls_score_net", 0.01), ("rpn_bbox_pred_net", 0.01), ("cls_score_net", 0.01), ("bbox_pred_net", 0.001)):
        m = getattr(net, name)
        n = m.weight.numel()
        assert abs(m.weight.std().item() / std - 1) <= 5 / np.sqrt(2 * n), name
        assert abs(m.weight.mean().item()) <= 5 * std / np.sqrt(n), name
        assert not m.bias.any()


def test_blob_sizes():
    a, b = det_test.blob_size(50, 72, 75, 125), det_test.blob_size(40, 96, 75, 125)
    assert a == (1.5, 75, 108) and b == (125.0 / 96.0, 52, 125)           # b: the MAX_SIZE branch (75 / 40 * 96 = 180 > 125)
    assert R.blob_size(50, 72, 75, 125) == a and R.blob_size(40, 96, 75, 125) == b
    for case, want in zip(CASES, (a, b)):
        assert G[case + "_blob"].shape == (1, 3, want[1], want[2])
        assert np.array_equal(G[case + "_im_info"], np.array([want[1], want[2], want[0]], dtype=np.float32))
    assert R.map_sizes(75) == (38, 19, 10, 5) and R.map_sizes(108) == (54, 27, 14, 7)
    assert R.map_sizes(52) == (26, 13, 7, 4) and R.map_sizes(125) == (63, 32, 16, 8)
    assert G["a_net_conv"].shape == (1, 1024, 5, 7) and G["b_net_conv"].shape == (1, 1024, 4, 8)
    assert det_test.blob_size(480, 640) == (1.25, 600, 800) and det_test.blob_size(300, 900)[1:] == (333, 1000)


def test_unsupported_requests():
    with pytest.raises(NotImplementedError):
        nets.resnetv1(34).create_architecture(K, tag="default")
    net = _net()
    blob = np.zeros((1, 32, 32, 3), dtype=np.float32)
    with pytest.raises(FlowtrackHipError):
        net.forward(blob, np.array([32, 32, 1], dtype=np.float32), None, mode="TRAIN")
    with pytest.raises(FlowtrackHipError):
        net.forward(blob, np.array([32, 32, 1], dtype=np.float32), np.zeros((1, 5), dtype=np.float32), mode="TEST")
    with pytest.raises(FlowtrackHipError):
        net.train_step({}, None)


def test_synthetic_weights_are_deterministic():
    again = synth.fill_detector_state_dict(_net().state_dict(), SEED)
    assert all(torch.equal(again[k], v) for k, v in _state_dict().items())
    assert not torch.equal(synth.fill_detector_state_dict(_net().state_dict(), SEED + 1)["cls_score_net.weight"], again["cls_score_net.weight"])
    f = synth.detector_frame(SEED, 50, 72)
    assert f.dtype == np.uint8 and f.shape == (50, 72, 3) and np.array_equal(f, _frame("a"))


# ---- the derived bounds against float32 runs of the references -----------------------------------------------------------------
def test_blob_bound_holds_for_float32():
    for case in CASES:
        frame = _frame(case)
        im_scale, Hb, Wb = R.blob_size(*frame.shape[:2], TARGET, MAX_SIZE)
        s = 1.0 / im_scale
        f32, f64 = (R.blob_ref(frame, R.PIXEL_MEANS, Hb, Wb, s, s, dt) for dt in (np.float32, np.float64))
        err, bound = np.abs(f32.astype(np.float64) - f64).max(), R.blob_bound(frame, R.PIXEL_MEANS)
        assert f32.dtype == np.float32 and 0 < err <= bound <= 1.3e-4, (err, bound)
        assert np.array_equal(f64.astype(np.float32), G[case + "_blob"])         # the golden's blob is this float64 form, rounded
    frame = _frame("a")
    ident = R.blob_ref(frame, R.PIXEL_MEANS, 50, 72, 1.0, 1.0, np.float32)
    assert np.array_equal(ident[0].transpose(1, 2, 0), (frame.astype(np.float64) - R.PIXEL_MEANS).astype(np.float32))


def test_softmax_bounds_hold_for_float32():
    x = synth.normal(SEED, "sm", (35, 18), std=3.0).numpy()
    x[0], x[1, :9], x[1, 9:] = 1.25, 60.0, -60.0
    f32, f64 = R.rpn_softmax_ref(x, 9, np.float32), R.rpn_softmax_ref(x, 9, np.float64)
    bound = R.softmax_bound(x.reshape(-1, 2, 9), 1).reshape(-1, 18)
    assert f32.dtype == np.float32 and np.all(np.abs(f32 - f64) <= bound) and bound.max() <= 2e-5
    assert np.all(f32[0] == 0.5) and np.isfinite(f32).all()
    for Kc in (1, 3, 81):
        s = synth.normal(SEED, f"cls{Kc}", (41, Kc), std=2.0).numpy()
        p32, p64 = (R.detections_ref(s, np.zeros((41, 4 * Kc), np.float32), np.zeros((41, 5), np.float32), R.BBOX_STDS, R.BBOX_MEANS, 1.0, 9, 9, dt)[0]
                    for dt in (np.float32, np.float64))
        assert np.all(np.abs(p32 - p64) <= R.softmax_bound(s, 1)) and abs(p64.sum(1) - 1).max() <= 1e-12


def test_mean_pool_bound_holds_for_float32():
    x = synth.normal(SEED, "mp", (3, 7, 7, 16), std=2.0).numpy()
    f32, f64 = R.mean_pool_ref(x, np.float32), R.mean_pool_ref(x, np.float64)
    assert f32.dtype == np.float32 and np.all(np.abs(f32 - f64) <= R.mean_pool_bound(x))
    assert np.abs(f64 - x.astype(np.float64).mean(axis=(1, 2))).max() <= 1e-14
    xi = 49.0 * np.floor(synth.uniform(SEED, "mpi", (3, 7, 7, 8), -20, 21).numpy())          # every partial result is an integer
    assert np.array_equal(R.mean_pool_ref(xi, np.float32), R.mean_pool_ref(xi, np.float64).astype(np.float32))
    h = x.astype(np.float16)
    assert np.all(np.abs(R.mean_pool_ref(h, np.float32).astype(np.float16).astype(np.float64) - R.mean_pool_ref(h, np.float64))
                  <= R.mean_pool_bound(h, np.float16))


def test_detections_bound_holds_for_float32():
    for case in CASES:
        rois, im_scale = G[case + "_rois"], float(G[case + "_im_info"][2])
        h, w = (int(v) for v in G[case + "_frame_hw"])
        raw = (G[case + "_bbox_pred"].reshape(-1, K, 4) / np.array(R.BBOX_STDS, dtype=np.float32)).reshape(-1, 4 * K).astype(np.float32)
        o32, o64 = (R.detections_ref(G[case + "_cls_score"], raw, rois, R.BBOX_STDS, R.BBOX_MEANS, im_scale, h, w, dt) for dt in (np.float32, np.float64))
        bound = R.detections_bound(raw, rois, R.BBOX_STDS, R.BBOX_MEANS, im_scale)
        assert np.array_equal(o32[1], o64[1]) and np.all(np.abs(o32[2].astype(np.float64) - o64[2]) <= bound) and bound.max() <= 1e-3
        assert np.abs(o64[2] - G[case + "_pred_boxes"]).max() <= 1e-5 and np.abs(o64[0] - G[case + "_scores"]).max() <= 1e-5
