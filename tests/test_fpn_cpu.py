"""FPN pose head, host side (no GPU): the functional restatement against the reference's recorded heat maps, the resize reference
against torch's own resize, and models.fpn's state_dict contract (tests/golden/fpn_golden.npz, written by make_fpn_golden.py)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_ref
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from flowtrack.pytorch_amd.pose import models


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "fpn_golden.npz"), allow_pickle=False)


def _fmt(sd):
    return ["%s %s %s" % (k, "x".join(str(d) for d in v.shape), v.dtype) for k, v in sd.items()]


def test_fixture_margins():
    """What make_fpn_golden.py asserted when it wrote the file: every map with score > 0 has a top-1 / top-2 margin of at least 4e-3."""
    g = _golden()
    assert float(g["min_margin"]) == 4e-3
    for B, H, W in g["shapes"]:
        tag = f"b{B}_{H}x{W}"
        live = g[tag + "_scores"][..., 0] > 0
        assert live.any() and (g[tag + "_margin"][live] >= 4e-3).all()


def test_fpn_forward_matches_reference():
    g = _golden()
    seed = int(g["seed"])
    sd = synth.fill_pose_state_dict(models.fpn("resnet50", 17, False).state_dict(), seed)
    for B, H, W in g["shapes"]:
        tag = f"b{B}_{H}x{W}"
        hm = fpn_ref.fpn_forward(sd, synth.pose_crops(seed, int(B), int(H), int(W)), depth=50)
        err = (hm - torch.from_numpy(g[tag + "_heatmaps"])).abs().max().item()
        print(f"fpn_forward {tag}: max abs vs the reference's heat maps {err:.3e}")
        assert tuple(hm.shape) == (B, 17, H // 4, W // 4) and err <= 1e-5
        assert np.array_equal(hm.flatten(2).argmax(2).numpy(), g[tag + "_idx"])


@pytest.mark.parametrize("case", fpn_ref.UPSAMPLE_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
def test_upsample_ref_vs_torch(case, scaled):
    """upsample_ac_ref against F.interpolate(mode='bilinear', align_corners=True) on fp32 data, held to the derived bound of an
    fp32 evaluation (upsample_ac_bound): the coordinate rule is torch's, so nothing but rounding separates the two."""
    name, N, C, hi, wi, ho, wo = case
    x = synth.normal(5, "fpn.up." + name, (N, C, hi, wi))
    scale = synth.uniform(5, "fpn.up.scale." + name, (C,), 0.5, 1.5) if scaled else None
    want, mag = fpn_ref.upsample_ac_ref(x, ho, wo, scale)
    got = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
    if scaled:
        got = got * scale.view(1, -1, 1, 1)
    bound = fpn_ref.upsample_ac_bound(want, mag, scale)
    ratio = ((got.double() - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{name} scaled={scaled}: worst error / bound {ratio:.3f}")
    assert tuple(want.shape) == (N, C, ho, wo) and ratio <= 1.0


def test_upsample_ref_exact_cases():
    """Where every weight is 0, 0.5 or 1 and the data are small integers the reference is exact: identity returns the input,
    out = 2 in - 1 returns the input on the even grid and the mean of two / four neighbours between."""
    x = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).reshape(2, 3, 5, 4) % 17 - 8
    same, _ = fpn_ref.upsample_ac_ref(x, 5, 4)
    assert torch.equal(same, x.double())
    up, _ = fpn_ref.upsample_ac_ref(x, 9, 7)
    assert torch.equal(up[:, :, ::2, ::2], x.double())
    assert torch.equal(up[:, :, 1::2, 1::2], (x[:, :, :-1, :-1] + x[:, :, :-1, 1:] + x[:, :, 1:, :-1] + x[:, :, 1:, 1:]).double() / 4)
    assert torch.equal(up.float(), F.interpolate(x, size=(9, 7), mode="bilinear", align_corners=True))


def test_state_dict_contract():
    g = _golden()
    m = models.fpn("resnet50", 17, False)
    assert _fmt(m.state_dict()) == list(g["state_dict_keys"])
    assert not any(k.startswith("deconv.") for k in m.state_dict())
    sd = synth.fill_pose_state_dict(m.state_dict(), 3)
    m2 = models.fpn("resnet50", 17, False)
    m2.load_state_dict(sd)
    back = m2.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # a torch-0.4 checkpoint has no num_batches_tracked
    old = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    models.fpn("resnet50", 17, False).load_state_dict(old)
    # a deconv checkpoint is not an FPN checkpoint
    with pytest.raises(RuntimeError):
        m2.load_state_dict(models.deconv("resnet50", 17, False).state_dict())


def test_init_net_follows_reference():
    """pose_fpn.py:89-104: lateral / top-down / heatmap convs N(0, 0.001^2), their BatchNorms (1, 0), the heatmap bias 0;
    the trunk convs keep resnet.py:38-49's kaiming_normal(fan_out)."""
    m = models.fpn("resnet101", 16, False)
    assert m.layers_cfg == [3, 4, 23, 3] and tuple(m.heatmap[2].weight.shape) == (16, 256, 1, 1)
    for name in ("latlayer1", "latlayer4"):
        w = getattr(m, name).weight
        assert abs(w.std().item() - 1e-3) < 1e-4 and abs(w.mean().item()) < 1e-4
    for top in (m.toplayer1, m.toplayer3):
        assert abs(top[2].weight.std().item() - 1e-3) < 1e-4
        assert bool((top[0].weight == 1).all()) and bool((top[0].bias == 0).all())
    assert abs(m.heatmap[2].weight.std().item() - 1e-3) < 2e-4 and bool((m.heatmap[2].bias == 0).all())
    w = m.layer1[0].conv2.weight
    assert abs(w.std().item() - (2.0 / (64 * 9)) ** 0.5) < 5e-3


def test_factory_refusals():
    for backbone in ("densenet121", "resnet18", "resnet", "hourglass"):
        with pytest.raises(FlowtrackHipError, match="resnet50 / resnet101 / resnet152"):
            models.fpn(backbone, 17, False)


def test_exact_mode_refuses_fpn():
    m = models.fpn("resnet50", 17, False).eval()
    m.keypoints_in_plan = True
    x = torch.zeros(1, 3, 64, 64)
    for call in (lambda: m.exact_submit(x), lambda: m.forward_keypoint_rows_exact(x), lambda: m.exact_submit_plan(None)):
        with pytest.raises(FlowtrackHipError, match="exact-arg-max mode is not available"):
            call()
    m.exact_in_plan = True
    with pytest.raises(FlowtrackHipError, match="exact-arg-max mode is not available"):
        m.plan_for(1, 64, 64)
