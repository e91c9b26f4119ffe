"""Lateral-deconv pose head, host side (no GPU): the functional restatement against the reference's recorded heat maps, models.pose's
state_dict contract and init_net (tests/golden/posenet_golden.npz, written by make_posenet_golden.py), the factory's refusals, and the
packed [taps | W2] layout of one top-down step multiplied out on the CPU."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posenet_ref
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from flowtrack.pytorch_amd.pose import models


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "posenet_golden.npz"), allow_pickle=False)


def _fmt(sd):
    return ["%s %s %s" % (k, "x".join(str(d) for d in v.shape), v.dtype) for k, v in sd.items()]


def test_fixture_margins():
    """What make_posenet_golden.py asserted when it wrote the file: every map with score > 0 has a top-1 / top-2 margin of at least 4e-3."""
    g = _golden()
    assert float(g["min_margin"]) == 4e-3
    assert [tuple(int(v) for v in s) for s in g["shapes"]] == [(2, 128, 96), (3, 64, 64)]
    for B, H, W in g["shapes"]:
        tag = f"b{B}_{H}x{W}"
        live = g[tag + "_scores"][..., 0] > 0
        assert live.any() and (g[tag + "_margin"][live] >= 4e-3).all()


def test_posenet_forward_matches_reference():
    g = _golden()
    seed = int(g["seed"])
    sd = synth.fill_pose_state_dict(models.pose("resnet50", 17, False).state_dict(), seed)
    for B, H, W in g["shapes"]:
        tag = f"b{B}_{H}x{W}"
        hm = posenet_ref.posenet_forward(sd, synth.pose_crops(seed, int(B), int(H), int(W)), depth=50)
        err = (hm - torch.from_numpy(g[tag + "_heatmaps"])).abs().max().item()
        print(f"posenet_forward {tag}: max abs vs the reference's heat maps {err:.3e}")
        assert tuple(hm.shape) == (B, 17, H // 4, W // 4) and err <= 1e-5
        assert np.array_equal(hm.flatten(2).argmax(2).numpy(), g[tag + "_idx"])


def test_state_dict_contract():
    g = _golden()
    m = models.pose("resnet50", 17, False)
    assert isinstance(m, models.LateralDeconvResnet) and m.full_stage_maps and not m.supports_exact
    assert _fmt(m.state_dict()) == list(g["state_dict_keys"])
    keys = set(m.state_dict())
    assert not any(k.startswith(("latlayer1", "toplayer", "deconv.")) for k in keys)
    assert not any(k.endswith(".bias") and k.startswith(("latlayer", "deconv1.2", "deconv2.2", "deconv3.2")) for k in keys)
    assert tuple(m.state_dict()["latlayer2.weight"].shape) == (256, 1024, 1, 1) and tuple(m.state_dict()["deconv1.0.weight"].shape) == (2048,)
    assert tuple(m.state_dict()["deconv1.2.weight"].shape) == (2048, 256, 4, 4) and "heatmap.2.bias" in keys
    sd = synth.fill_pose_state_dict(m.state_dict(), 3)
    m2 = models.pose("resnet50", 17, False)
    m2.load_state_dict(sd)                      # a reference-keyed state dict loads strict
    back = m2.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # a torch-0.4 checkpoint has no num_batches_tracked
    old = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    models.pose("resnet50", 17, False).load_state_dict(old)
    # neither a deconv nor an FPN checkpoint is a lateral-deconv checkpoint
    for other in (models.deconv, models.fpn):
        with pytest.raises(RuntimeError):
            m2.load_state_dict(other("resnet50", 17, False).state_dict())


def test_init_net_follows_reference():
    """pose_net.py:69-91: lateral / deconv / heatmap weights N(0, 0.001^2), the head's BatchNorms (1, 0), the heatmap bias 0;
    the trunk convs keep resnet.py:38-49's kaiming_normal(fan_out)."""
    m = models.pose("resnet101", 16, False)
    assert m.layers_cfg == [3, 4, 23, 3] and tuple(m.heatmap[2].weight.shape) == (16, 256, 1, 1)
    for name in ("latlayer2", "latlayer3", "latlayer4"):
        w = getattr(m, name).weight
        assert abs(w.std().item() - 1e-3) < 1e-4 and abs(w.mean().item()) < 1e-4 and getattr(m, name).bias is None
    for dc in (m.deconv1, m.deconv2, m.deconv3):
        assert abs(dc[2].weight.std().item() - 1e-3) < 1e-4 and abs(dc[2].weight.mean().item()) < 1e-4 and dc[2].bias is None
        assert bool((dc[0].weight == 1).all()) and bool((dc[0].bias == 0).all())
    assert (m.deconv1[0].weight.numel(), m.deconv2[0].weight.numel(), m.deconv3[0].weight.numel()) == (2048, 256, 256)
    assert bool((m.heatmap[0].weight == 1).all()) and bool((m.heatmap[0].bias == 0).all())
    assert abs(m.heatmap[2].weight.std().item() - 1e-3) < 2e-4 and bool((m.heatmap[2].bias == 0).all())
    w = m.layer1[0].conv2.weight
    assert abs(w.std().item() - (2.0 / (64 * 9)) ** 0.5) < 5e-3


def test_factory_refusals():
    for backbone in ("densenet121", "resnet18", "resnet", "hourglass"):
        with pytest.raises(FlowtrackHipError, match="resnet50 / resnet101 / resnet152"):
            models.pose(backbone, 17, False)
    with pytest.raises(FlowtrackHipError, match="reference itself cannot build"):
        models.pose("densenet121", 17, False)


def test_exact_mode_refuses_posenet():
    m = models.pose("resnet50", 17, False).eval()
    m.keypoints_in_plan = True
    x = torch.zeros(1, 3, 64, 64)
    for call in (lambda: m.exact_submit(x), lambda: m.forward_keypoint_rows_exact(x), lambda: m.exact_submit_plan(None)):
        with pytest.raises(FlowtrackHipError, match="exact-arg-max mode is not available"):
            call()
    m.exact_in_plan = True
    with pytest.raises(FlowtrackHipError, match="exact-arg-max mode is not available"):
        m.plan_for(1, 64, 64)


@pytest.mark.parametrize("cin,cin2,cout,pads", [(5, 3, 4, (8, 8, 8)), (6, 7, 3, (6, 7, 3))], ids=["padded", "tight"])
def test_packed_taps_w2_layout(cin, cin2, cout, pads):
    """The [taps | W2] layout of one top-down step (include/flowtrack_hip.h), restated in numpy and multiplied out in float64 on
    small-integer data, equals conv_transpose2d(4,2,1) + conv2d(1x1) on a 2 x 3 map exactly; padding columns / rows are zero and every
    phase carries the same W2 block."""
    cin_pad, cin2_pad, cout_pad = pads
    rng = np.random.RandomState(11)
    wt = rng.randint(-3, 4, size=(cin, cout, 4, 4)).astype(np.float64)
    w2 = rng.randint(-3, 4, size=(cout, cin2, 1, 1)).astype(np.float64)
    x = rng.randint(-4, 5, size=(2, cin, 2, 3)).astype(np.float64)
    x2 = rng.randint(-4, 5, size=(2, cin2, 4, 6)).astype(np.float64)
    packed = posenet_ref.pack_taps_w2(wt, w2, cin_pad, cin2_pad, cout_pad)
    assert packed.shape == (4, cout_pad, 4 * cin_pad + cin2_pad)
    for ph in range(4):
        assert np.array_equal(packed[ph, :cout, 4 * cin_pad:4 * cin_pad + cin2], w2[:, :, 0, 0])
        assert not packed[ph, cout:].any() and not packed[ph, :, 4 * cin_pad + cin2:].any()
        for t in range(4):
            assert not packed[ph, :, t * cin_pad + cin:(t + 1) * cin_pad].any()
    got = posenet_ref.packed_step_ref(packed, x, x2, cin_pad, cout)
    want = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(wt), stride=2, padding=1) + F.conv2d(torch.from_numpy(x2), torch.from_numpy(w2))
    assert got.shape == (2, cout, 4, 6) and np.array_equal(got, want.numpy())
