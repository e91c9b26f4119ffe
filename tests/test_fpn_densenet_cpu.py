"""FPN pose model on DenseNet trunks, host side (no GPU): the functional restatement against the reference's recorded heat maps
(tests/golden/fpn_densenet_golden.npz, written by make_fpn_densenet_golden.py), models.fpn_densenet's state_dict / init / refusal
contract, the weight packer's layout, and the float64 restatement of ft_preact_conv1x1_fwd against torch's own layers."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_densenet_ref as dref
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from flowtrack.pytorch_amd.hip_ops import pack_preact_weights
from flowtrack.pytorch_amd.pose import models


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "fpn_densenet_golden.npz"), allow_pickle=False)


def _fmt(sd):
    return ["%s %s %s" % (k, "x".join(str(d) for d in v.shape), v.dtype) for k, v in sd.items()]


def test_fixture_conditions():
    """What make_fpn_densenet_golden.py asserted when it wrote the file: heat maps within +-16, dense-block outputs within fp16
    headroom, every map with score > 0 with a top-1 / top-2 margin of at least 4e-3."""
    g = _golden()
    assert float(g["min_margin"]) == 4e-3 and float(g["block_max"]) <= 1024
    assert [tuple(s) for s in g["shapes"]] == [(2, 128, 96), (3, 64, 64)]
    for B, H, W in g["shapes"]:
        tag = f"b{B}_{H}x{W}"
        live = g[tag + "_scores"][..., 0] > 0
        assert live.any() and (g[tag + "_margin"][live] >= 4e-3).all() and np.abs(g[tag + "_heatmaps"]).max() <= 16


def test_restatement_matches_reference():
    g = _golden()
    seed = int(g["seed"])
    sd = synth.fill_densenet_state_dict(models.fpn_densenet("densenet121", 17, False).state_dict(), seed)
    for B, H, W in g["shapes"]:
        tag = f"b{B}_{H}x{W}"
        hm = dref.fpn_densenet_forward(sd, synth.pose_crops(seed, int(B), int(H), int(W)), depth=121)
        err = (hm - torch.from_numpy(g[tag + "_heatmaps"])).abs().max().item()
        print(f"fpn_densenet_forward {tag}: max abs vs the reference's heat maps {err:.3e}")
        assert tuple(hm.shape) == (B, 17, H // 4, W // 4) and err <= 1e-5
        assert np.array_equal(hm.flatten(2).argmax(2).numpy(), g[tag + "_idx"])


def test_state_dict_contract():
    g = _golden()
    m = models.fpn_densenet("densenet121", 17, False)
    want = list(g["state_dict_keys"])
    assert len(want) == 754 and _fmt(m.state_dict()) == want
    assert m.planes == [256, 512, 1024, 1024] == dref.planes(121)
    sd = synth.fill_densenet_state_dict(m.state_dict(), 3)
    m2 = models.fpn_densenet("densenet121", 17, False)
    m2.load_state_dict(sd)
    back = m2.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):       # a ResNet FPN checkpoint is not a DenseNet one
        m2.load_state_dict(models.fpn("resnet50", 17, False).state_dict())


@pytest.mark.parametrize("depth", [169, 201])
def test_other_depths_follow_block_config(depth):
    """No fixture for 169 / 201: the key count and `planes` follow from densenet.py:150-153's block configs.  Per dense layer 2 convs +
    2 BatchNorms (5 entries each) = 12 entries, per transition 6, conv0 + norm0 + norm5 = 11, the head 4 lateral + 3 x (5 + 1) + 5 + 2."""
    init, growth, cfg = dref.DENSENET[depth]
    m = models.fpn_densenet(f"densenet{depth}", 17, False)
    assert len(m.state_dict()) == 12 * sum(cfg) + 6 * 3 + 11 + 4 + 18 + 7
    assert m.planes == dref.planes(depth)
    assert tuple(m.latlayer1.weight.shape) == (256, m.planes[3], 1, 1) and tuple(m.latlayer4.weight.shape) == (256, m.planes[0], 1, 1)
    last = getattr(m.denseblock4, f"denselayer{cfg[3]}")
    assert tuple(last.conv1.weight.shape) == (4 * growth, m.planes[3] - growth, 1, 1) and tuple(last.conv2.weight.shape) == (growth, 4 * growth, 3, 3)
    assert tuple(m.norm5.weight.shape) == (m.planes[3],)


def test_checkpoint_key_rewrite(tmp_path):
    """densenet.py:126-139: `features.` stripped, `norm.1` -> `norm1` (torchvision's old DenseNet keys), loaded strict=False."""
    m = models.fpn_densenet("densenet121", 17, False)
    w = torch.full_like(m.denseblock1.denselayer1.norm1.weight, 0.375)
    c = torch.full_like(m.denseblock2.denselayer3.conv2.weight, -0.5)
    c0 = torch.full_like(m.conv0.weight, 0.25)
    ckpt = {"features.denseblock1.denselayer1.norm.1.weight": w, "features.denseblock2.denselayer3.conv.2.weight": c,
            "features.conv0.weight": c0, "classifier.weight": torch.zeros(1000, 1024)}
    assert set(models.FpnDensenet.rewrite_checkpoint_keys(ckpt)) == {"denseblock1.denselayer1.norm1.weight", "denseblock2.denselayer3.conv2.weight",
                                                                      "conv0.weight", "classifier.weight"}
    path = tmp_path / "densenet121.pth"
    torch.save(ckpt, str(path))
    m.init_net(str(path))
    assert torch.equal(m.denseblock1.denselayer1.norm1.weight, w) and torch.equal(m.denseblock2.denselayer3.conv2.weight, c)
    assert torch.equal(m.conv0.weight, c0)
    assert abs(m.latlayer2.weight.std().item() - 1e-3) < 1e-4         # (the head's init runs behind the load, as in the reference)


def test_init_net_follows_reference():
    """pose_fpn.py:153-168: lateral / top-down / heatmap convs N(0, 0.001^2), their BatchNorms (1, 0), the heatmap bias 0;
    densenet.py:141-148: trunk convs kaiming_normal (fan_in), BatchNorms (1, 0)."""
    m = models.fpn_densenet("densenet121", 16, False)
    assert tuple(m.heatmap[2].weight.shape) == (16, 256, 1, 1)
    for name in ("latlayer1", "latlayer4"):
        w = getattr(m, name).weight
        assert abs(w.std().item() - 1e-3) < 1e-4 and abs(w.mean().item()) < 1e-4
    for top in (m.toplayer1, m.toplayer3):
        assert abs(top[2].weight.std().item() - 1e-3) < 1e-4
        assert bool((top[0].weight == 1).all()) and bool((top[0].bias == 0).all())
    assert abs(m.heatmap[2].weight.std().item() - 1e-3) < 2e-4 and bool((m.heatmap[2].bias == 0).all())
    w = m.denseblock3.denselayer5.conv2.weight
    assert abs(w.std().item() - (2.0 / (128 * 9)) ** 0.5) < 2e-3
    n = m.denseblock3.denselayer5.norm1
    assert bool((n.weight == 1).all()) and bool((n.bias == 0).all())


def test_factory_refusals():
    for backbone in ("resnet50", "densenet122", "densenet"):
        with pytest.raises(FlowtrackHipError, match="densenet121 / densenet169 / densenet201"):
            models.fpn_densenet(backbone, 17, False)
    with pytest.raises(FlowtrackHipError, match="growth rate 48.*densenet121 / densenet169 / densenet201"):
        models.fpn_densenet("densenet161", 17, False)
    with pytest.raises(FlowtrackHipError, match="resnet50 / resnet101 / resnet152"):
        models.fpn("densenet121", 17, False)


def test_exact_mode_and_small_inputs_refused():
    m = models.fpn_densenet("densenet121", 17, False).eval()
    m.keypoints_in_plan = True
    with pytest.raises(FlowtrackHipError, match="exact-arg-max mode is not available"):
        m.exact_submit(torch.zeros(1, 3, 64, 64))
    with pytest.raises(FlowtrackHipError, match="multiples of 32 and at least 64"):
        m._check_input_size(32, 64)
    m.dense_layer_form = "fused"
    with pytest.raises(FlowtrackHipError, match="dense_layer_form"):
        m._record_net(None, torch.zeros(1, 3, 64, 64), torch.float32, torch.device("cpu"))


def test_pack_layout():
    """The fp16 operand order stated in include/flowtrack_hip.h: element (g, c, s, lane, e) = W[32 g + (lane & 31)][64 c + 32 (lane >> 5)
    + 8 s + e], zeros past Cin; fp32: the weights as they are."""
    cout, cin = 64, 160
    w = (torch.arange(cout * cin, dtype=torch.float32).reshape(cout, cin, 1, 1) % 2039) - 1000       # exact in fp16
    p = pack_preact_weights(w, torch.float16, "cpu")
    assert p.dtype == torch.float16 and tuple(p.shape) == (2, 3, 4, 2, 32, 8) and p.is_contiguous()
    flat = p.reshape(2, 3, 4, 64, 8)
    for g, c, s, lane, e in ((0, 0, 0, 0, 0), (1, 2, 3, 63, 7), (1, 1, 2, 37, 5), (0, 2, 1, 31, 0), (0, 2, 0, 32, 0)):
        k = 64 * c + 32 * (lane >> 5) + 8 * s + e
        want = float(w[32 * g + (lane & 31), k, 0, 0]) if k < cin else 0.0
        assert float(flat[g, c, s, lane, e]) == want, (g, c, s, lane, e)
    assert torch.equal(pack_preact_weights(w, torch.float32, "cpu"), w.reshape(cout, cin))
    with pytest.raises(FlowtrackHipError, match="multiples of 32"):
        pack_preact_weights(torch.zeros(48, 64), torch.float16, "cpu")


@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pool"])
def test_preact_ref_vs_torch(pool):
    """preact_conv1x1_ref against F.conv2d(F.relu(F.batch_norm(x))) (+ norm2 + ReLU behind it), and pooled against
    F.avg_pool2d(conv(...)) — the order the reference computes a transition in: the pool commutes with the 1x1 conv, so only fp32
    rounding separates the two.  Held to the restatement's own fp32 bound plus the same allowance for torch's fp32 evaluation."""
    N, H, W, cin, cout = 2, 5, 7, 40, 32
    x = synth.normal(9, "preact.x", (N, cin, H, W))
    w = synth.normal(9, "preact.w", (cout, cin, 1, 1), std=cin ** -0.5)
    bn1 = [synth.uniform(9, "preact.g1", (cin,), 0.5, 1.5), synth.normal(9, "preact.b1", (cin,), std=0.3),
           synth.normal(9, "preact.m1", (cin,), std=0.3), synth.uniform(9, "preact.v1", (cin,), 0.5, 1.5)]
    bn2 = [synth.uniform(9, "preact.g2", (cout,), 0.5, 1.5), synth.normal(9, "preact.b2", (cout,), std=0.3),
           synth.normal(9, "preact.m2", (cout,), std=0.3), synth.uniform(9, "preact.v2", (cout,), 0.5, 1.5)]

    def fold(g, b, m, v):
        s = g.double() / torch.sqrt(v.double() + 1e-5)
        return s, b.double() - m.double() * s
    a = F.relu(F.batch_norm(x, bn1[2], bn1[3], bn1[0], bn1[1], False, 0.0, 1e-5))
    y = F.conv2d(a, w)
    if pool:
        got = F.avg_pool2d(y, 2, 2)
        post = (None, None)
    else:
        got = F.relu(F.batch_norm(y, bn2[2], bn2[3], bn2[0], bn2[1], False, 0.0, 1e-5))
        post = fold(*bn2)
    want, bound = dref.preact_conv1x1_ref(x.permute(0, 2, 3, 1), w.reshape(cout, cin), *fold(*bn1), post[0], post[1], pool=pool, relu=not pool)
    got = got.permute(0, 2, 3, 1).double()
    ratio = ((got - want).abs() / (2 * bound + 4 * 2.0 ** -24 * want.abs()).clamp_min(1e-300)).max().item()
    print(f"preact_conv1x1_ref pool={pool}: worst |torch - ref| / allowance {ratio:.3f}")
    assert tuple(want.shape) == ((N, H // 2, W // 2, cout) if pool else (N, H, W, cout)) and ratio <= 1.0
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-4


def test_preact_ref_integer_exact():
    """Small integers, power-of-two scales: every product and sum is exact, so the restatement equals integer arithmetic and its
    pooled form equals pooling the un-pooled result."""
    from exact_preact_cases import exact_case, exact_want
    for pool in (False, True):
        c = exact_case("cpu", 1, 5, 7, 64, 32, pool)
        want, _ = dref.preact_conv1x1_ref(c["x"], c["w"], c["pre_scale"], c["pre_shift"], c["post_scale"], c["post_shift"], pool=pool, relu=True)
        assert torch.equal(want, exact_want(c, pool, True))
