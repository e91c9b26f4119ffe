"""Stacked hourglass, host side (no GPU): the functional restatement against the reference's recorded heat maps, the kernel
references against torch's own ops, models.hg's state_dict contract, init and refusals (tests/golden/hg_golden.npz, written by
make_hg_golden.py)."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hourglass_ref
from conftest import GOLDEN
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from flowtrack.pytorch_amd.pose import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "hg_golden.npz"), allow_pickle=False)


def _configs():
    return [tuple(int(v) for v in c) for c in _golden()["configs"]]


def _fmt(sd):
    return ["%s %s %s" % (k, "x".join(str(d) for d in v.shape), v.dtype) for k, v in sd.items()]


def test_fixture_conditions():
    """What make_hg_golden.py asserted when it wrote the file: the largest activation is <= 4096 and at least 3/4 of the last stack's
    live maps have a margin >= 2 tol, at every configuration."""
    g = _golden()
    assert _configs() == [(8, 2, 64, 64), (8, 2, 96, 80), (2, 2, 96, 80)]
    for cfg in _configs():
        tag = "s%d_b%d_%dx%d" % cfg
        hms = g[tag + "_heatmaps"]
        assert hms.shape == (cfg[0], cfg[1], 17, cfg[2] // 4, cfg[3] // 4) and g[tag + "_margin"].shape == hms.shape[:3]
        assert float(g[tag + "_peak"]) <= 4096.0
        live = g[tag + "_scores"][..., 0] > 0
        tol = hourglass_ref.stack_tol(hms[-1].max() - hms[-1].min())
        assert (g[tag + "_margin"][-1][live] >= 2 * tol).sum() >= 0.75 * live.sum() > 0


@pytest.mark.parametrize("cfg", [(8, 2, 64, 64), (8, 2, 96, 80), (2, 2, 96, 80)], ids=lambda c: "s%d_b%d_%dx%d" % c)
def test_hg_forward_matches_reference(cfg):
    g = _golden()
    S, B, H, W = cfg
    tag = "s%d_b%d_%dx%d" % cfg
    seed = int(g["seed"])
    sd = synth.fill_hg_state_dict(models.hg(17, S).state_dict(), seed)
    out, peak = hourglass_ref.hg_forward(sd, synth.pose_crops(seed, B, H, W), S, return_peak=True)
    gold = g[tag + "_heatmaps"]
    assert len(out) == S and peak <= 4096.0
    for i, hm in enumerate(out):
        rng = float(gold[i].max() - gold[i].min())
        err = (hm - torch.from_numpy(gold[i])).abs().max().item()
        assert tuple(hm.shape) == (B, 17, H // 4, W // 4) and err <= 1e-5 * rng, f"stack {i}: {err:.3e} on a range of {rng:.3e}"
    assert np.array_equal(out[-1].flatten(2).argmax(2).numpy(), g[tag + "_idx"])


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 5, 7, 20), (1, 3, 2, 16), (2, 6, 5, 24)], ids=str)
def test_down_ref_vs_torch(shape):
    """down_ref is nn.MaxPool2d(2, stride=2): an odd last row / column takes no part."""
    x = synth.normal(5, "hg.down", shape)
    x[:, shape[1] - 1 if shape[1] % 2 else shape[1]:] = 1e9
    x[:, :, shape[2] - 1 if shape[2] % 2 else shape[2]:] = 1e9
    want = F.max_pool2d(x.permute(0, 3, 1, 2), kernel_size=2, stride=2).permute(0, 2, 3, 1)
    got = torch.from_numpy(hourglass_ref.down_ref(x.numpy()))
    assert torch.equal(got, want) and not bool((got == 1e9).any())
    s, b = np.array([0.5, -2.0] * (shape[3] // 2)), np.arange(shape[3]) * 0.5 - 2
    xi = torch.round(x.clamp(-64, 64))
    assert torch.equal(torch.from_numpy(hourglass_ref.affine_relu_exact(xi.numpy(), s, b, np.float32)),
                       F.relu(xi * torch.from_numpy(s).float() + torch.from_numpy(b).float()))


@pytest.mark.parametrize("case", [(1, 8, 1, 1, 2, 2), (2, 20, 1, 1, 3, 2), (2, 20, 2, 3, 5, 6), (1, 16, 3, 2, 6, 5), (2, 8, 8, 6, 16, 12), (2, 8, 5, 6, 5, 6)],
                         ids=lambda c: "%dx%d_%dx%d" % c[2:])
def test_up_ref_vs_torch(case):
    """up_ref against F.interpolate(mode='bilinear', align_corners=True) + skip on fp32 data, held to the derived bound."""
    N, C, hl, wl, H, W = case
    skip, low = synth.normal(5, "hg.up.skip", (N, H, W, C)), synth.normal(5, "hg.up.low", (N, hl, wl, C))
    want, mag = hourglass_ref.up_ref(skip, low)
    got = (F.interpolate(low.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True) + skip.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    ratio = ((got.double() - want).abs() / hourglass_ref.up_bound(want, mag, fp16=False).clamp_min(1e-300)).max().item()
    assert tuple(want.shape) == (N, H, W, C) and ratio <= 1.0
    if (hl, wl) == (H, W):
        assert torch.equal(want, skip.double() + low.double())


@pytest.mark.parametrize("S", [8, 2])
def test_state_dict_contract(S):
    g = _golden()
    m = models.hg(num_classes=17, num_stacks=S)
    assert m.num_blocks == 8 // S and m.supports_exact is False and m.fuse_seams is True
    assert _fmt(m.state_dict()) == list(g[f"state_dict_keys_s{S}"])
    sd = synth.fill_hg_state_dict(m.state_dict(), 3)
    m2 = models.hg(17, S)
    m2.load_state_dict(sd, strict=True)
    back = m2.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # a torch-0.4 checkpoint has no num_batches_tracked
    models.hg(17, S).load_state_dict({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    with pytest.raises(RuntimeError):
        m2.load_state_dict(models.hg(17, 4).state_dict())


def test_init_follows_reference():
    """hourglass.py:166-173: kaiming_normal(fan_out, relu) on every conv, bias 0, BatchNorm (1, 0)."""
    m = models.hg(16, 4)
    assert m.num_blocks == 2 and tuple(m.heatmap[3].weight.shape) == (16, 256, 1, 1) and len(m.proj_) == len(m.heatmap_) == 3
    for conv, fan_out in ((m.pre[0], 64 * 49), (m.hg[1].hg[0][3][1].branch[3], 128 * 9), (m.res1[0].shortcut, 256), (m.heatmap_[0], 256)):
        assert abs(conv.weight.std().item() / (2.0 / fan_out) ** 0.5 - 1) < 0.05 and bool((conv.bias == 0).all())
    for bn in (m.pre[1], m.hg[0].hg[3][0][0].preact[0], m.proj[2][1]):
        assert bool((bn.weight == 1).all()) and bool((bn.bias == 0).all())
    assert not hasattr(m.res1[0], "preact") and m.res2[0].shortcut is None


def test_fill_hg_state_dict_gains():
    sd = synth.fill_hg_state_dict(models.hg(17, 8).state_dict(), 1)
    for key, gain, fan_in in (("hg.3.hg.2.1.0.branch.6.weight", 0.03, 128), ("proj_.0.weight", 0.03, 256), ("heatmap_.6.weight", 0.03, 17),
                              ("heatmap.7.weight", 1.0, 256), ("hg.0.hg.0.3.0.branch.3.weight", 2.0, 128 * 9), ("res1.0.shortcut.weight", 2.0, 64)):
        assert abs(sd[key].std().item() / (gain / fan_in) ** 0.5 - 1) < 0.06, key


def test_factory_and_size_refusals():
    for bad in (0, 9, -1, 2.0, "8", None, True):
        with pytest.raises(FlowtrackHipError, match="num_stacks"):
            models.hg(17, bad)
    m = models.hg(17, 8)
    for H, W in ((62, 64), (64, 66), (60, 64), (64, 32), (0, 64)):
        with pytest.raises(FlowtrackHipError, match="multiples of 4 and at least 64"):
            m._check_input_size(H, W)
    for H, W in ((64, 64), (96, 80), (256, 192), (68, 100)):
        m._check_input_size(H, W)


def test_exact_mode_refuses_hg():
    m = models.hg(17, 8).eval()
    m.keypoints_in_plan = True
    x = torch.zeros(1, 3, 64, 64)
    for call in (lambda: m.exact_submit(x), lambda: m.forward_keypoint_rows_exact(x)):
        with pytest.raises(FlowtrackHipError, match="exact-arg-max mode is not available"):
            call()


def test_header_declares_the_seam_kernels():
    text = open(os.path.join(ROOT, "include", "flowtrack_hip.h")).read()
    for name in ("ft_hourglass_down_fwd", "ft_hourglass_up_fwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and name in _lib.EXPORTED_SYMBOLS
    assert "hourglass_ops.hip" in open(os.path.join(ROOT, "flowtrack", "pytorch_amd", "build.py")).read()
