"""models.fpn_densenet on the GPU against the reference's recorded heat maps (tests/golden/fpn_densenet_golden.npz) and the live CPU
restatement (tests/fpn_densenet_ref.py::fpn_densenet_forward): fp32 parity and integer-exact arg-max at both golden shapes with the
launch list checked, the fp16 mode in the form of test_pose_fp16_vs_fp32_oracle, both forms of a dense layer's first launch against
each other, densenet169 (another block config, no fixture) against the live restatement, the flip plan, the pose tool and PoseRunner.

Measured on an MI355X: fp32 max abs against the fixture 7.6e-06 (2 x 128x96) and 7.0e-06 (3 x 64x64) on heat maps of range 18, scores
4.3e-06, smallest margin of a map with score > 0 8.9e-03 / 4.8e-03; block outputs 2.6e-06 at most on values up to 7.3; the two
dense-layer forms 5.7e-06 apart; densenet169 6.7e-06; fp16 at 2 x 128x96 8.3e-03 on a range of 17.7 = 0.47e-3 of the range = 0.16 of
the 3e-3 guard (the guard stays), arg-max identical on every map."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flip_ref
import fpn_densenet_ref as dref
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.pose import models
from oracle import keypoints_ref, pose_ref

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "fpn_densenet_golden.npz"), allow_pickle=False)
SEED = int(G["seed"])
SHAPES = [tuple(int(v) for v in s) for s in G["shapes"]]            # (2, 128, 96), (3, 64, 64)
SHAPE_IDS = ["x".join(str(v) for v in s) for s in SHAPES]
N_PREACT = 58 + 3 + 1          # densenet121: one per dense layer, one per transition, norm5 + latlayer1


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _state_dict(depth=121):
    return synth.fill_densenet_state_dict(models.fpn_densenet(f"densenet{depth}", num_classes=17, pretrained=False).state_dict(), SEED)


def _new_model(dtype, form="preact", depth=121):
    m = models.fpn_densenet(f"densenet{depth}", num_classes=17, pretrained=False)
    m.load_state_dict(_state_dict(depth))
    m = m.cuda().eval()
    m.compute_dtype, m.dense_layer_form = dtype, form
    return m


@functools.lru_cache(maxsize=None)
def _model(dtype, form="preact"):
    return _new_model(dtype, form)


@functools.lru_cache(maxsize=None)
def _live(shape):
    """(x, fpn_densenet_forward(x)) on the CPU, once per shape."""
    x = synth.pose_crops(SEED, *shape)
    return x, dref.fpn_densenet_forward(_state_dict(), x, depth=121)


def _tag(shape):
    return "b%d_%dx%d" % shape


def _check_fp32(hm, shape, what):
    """<= 1e-3 max-abs against the fixture and the live restatement; arg-max integer-exact on every map with score > 0, scores <= 1e-3."""
    tag = _tag(shape)
    gold = torch.from_numpy(G[tag + "_heatmaps"])
    err_gold = (hm - gold).abs().max().item()
    err_live = (hm - _live(shape)[1]).abs().max().item()
    _, scores, idx = keypoints_ref.max_preds_ref(hm.numpy())
    live = G[tag + "_scores"][..., 0] > 0
    err_score = np.abs(scores - G[tag + "_scores"]).max()
    print(f"{what} {tag}: max abs vs fixture {err_gold:.3e}, vs live restatement {err_live:.3e}, scores {err_score:.3e}, "
          f"{int(live.sum())} live maps, smallest live margin {G[tag + '_margin'][live].min():.3e}")
    assert tuple(hm.shape) == tuple(gold.shape)
    assert err_gold <= 1e-3 and err_live <= 1e-3 and err_score <= 1e-3
    assert np.array_equal(idx[live], G[tag + "_idx"][live]), "arg-max differs from the reference's on a map with score > 0"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fpn_densenet_fp32_parity(hip_lib, shape):
    x, _ = _live(shape)
    m = _model(torch.float32)
    hm = m(x.cuda())
    _check_fp32(hm.cpu(), shape, "fp32")
    plan = m._last_plan
    names = [c[0] for c in plan.prog.calls]
    assert names.count("ft_preact_conv1x1_fwd") == N_PREACT and names.count("ft_upsample_bilinear_ac_fwd") == 3
    assert "ft_scale_shift_act_nhwc_fwd" in names           # (fp32 only: the stem's pooled map into block 1's window)
    for li, c in ((1, 256), (2, 512), (3, 1024), (4, 1024)):
        v = plan.stages[f"layer{li}"]
        assert (v.H, v.W, v.C) == (shape[1] // (2 << li), shape[2] // (2 << li), c)
    for stage in ("p5", "p4", "p3", "p2"):
        assert stage in plan.stages
    again = m(x.cuda())                                  # the captured graph
    assert plan.runs >= 2 and plan.prog.graph_exec is not None and torch.equal(_bits(again), _bits(hm))


def test_fpn_densenet_stage_maps(hip_lib):
    """The block buffers ARE the concatenations: layer1..layer4 against the restatement's raw block outputs, p5..p3 against its maps, p2 against its activated map."""
    shape = SHAPES[1]
    x, _ = _live(shape)
    _, feats = dref.fpn_densenet_forward(_state_dict(), x, depth=121, return_features=True)
    # (the plan's p2 carries heatmap.0's BatchNorm + ReLU, folded into toplayer3's epilogue: only the heat-map conv reads it)
    feats["p2"] = F.relu(pose_ref._bn(_state_dict(), "heatmap.0", feats["p2"]))
    m = _model(torch.float32)
    m(x.cuda())
    for name, want in feats.items():
        v = m._last_plan.stages[name]
        got = v.t[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).float().cpu()
        err = (got - want).abs().max().item()
        print(f"stage {name}: {tuple(want.shape)} max abs {err:.3e} on values up to {want.abs().max().item():.2f}")
        assert err <= 1e-3


def test_fpn_densenet_fp16_vs_fp32_reference(hip_lib):
    """The form of test_pose_fp16_vs_fp32_oracle at 2 x 128x96: max-abs error against the fp32 CPU reference <= 3e-3 of the
    heat-map range (the project's guard for the fp16 mode), >= 97 % identical arg-max, every mismatch a near-tie (margin <= 2 err)."""
    shape = SHAPES[0]
    x, want = _live(shape)
    tag = _tag(shape)
    m = _model(torch.float16)
    hm = m(x.cuda()).cpu()
    err = (hm - want).abs().max().item()
    rng = (want.max() - want.min()).item()
    _, _, idx = keypoints_ref.max_preds_ref(hm.numpy())
    same = idx == G[tag + "_idx"]
    print(f"fpn_densenet fp16 {tag}: max abs {err:.3e} on a range of {rng:.3f} = {err / rng:.3e} of the range = {err / (3e-3 * rng):.3f} of the guard; "
          f"arg-max identical {same.mean():.4f}")
    assert err <= 3e-3 * rng, f"fp16 heatmap error {err:.3e} vs range {rng:.2f}"
    assert same.mean() >= 0.97, f"only {same.mean():.3f} of arg-max indices match"
    assert np.all(G[tag + "_margin"][~same] <= 2 * err + 1e-6), "an arg-max flip that is not explained by a near-tie"
    assert torch.equal(_bits(m(x.cuda()).cpu()), _bits(hm))
    names = [c[0] for c in m._last_plan.prog.calls]
    assert names.count("ft_preact_conv1x1_fwd") == N_PREACT and "ft_scale_shift_act_nhwc_fwd" not in names and "ft_maxpool3x3s2_fwd" not in names


def test_dense_layer_forms_agree(hip_lib):
    """"preact" and "affine+igemm" pinned in turn: the same network to the fp32 bar; the second writes the activated copies."""
    shape = SHAPES[1]
    x, _ = _live(shape)
    a = _model(torch.float32)(x.cuda()).cpu()
    m = _new_model(torch.float32, "affine+igemm")
    b = m(x.cuda()).cpu()
    names = [c[0] for c in m._last_plan.prog.calls]
    assert names.count("ft_preact_conv1x1_fwd") == 3 + 1 and names.count("ft_scale_shift_act_nhwc_fwd") == 58 + 1
    err = (a - b).abs().max().item()
    print(f"dense-layer forms, fp32 {_tag(shape)}: max abs difference {err:.3e}")
    assert err <= 1e-3
    _check_fp32(b, shape, "affine+igemm")
    # unpinned: both forms are recorded as a choice, the first-call benchmark keeps one per shape, the result is the same network
    m = _new_model(torch.float32, None)
    c = m(x.cuda()).cpu()
    names = [c_[0] for c_ in m._last_plan.prog.calls]
    assert not any(n.startswith("__") for n in names)
    assert names.count("ft_preact_conv1x1_fwd") + names.count("ft_scale_shift_act_nhwc_fwd") - 1 == N_PREACT
    assert (a - c).abs().max().item() <= 1e-3


def test_fpn_densenet169_vs_restatement(hip_lib):
    """Another block config ([6, 12, 32, 32]: 1280 / 1664 channels in blocks 3 / 4), no fixture: 1 x 64x64 fp32 against the live restatement."""
    x = synth.pose_crops(SEED, 1, 64, 64)
    want = dref.fpn_densenet_forward(_state_dict(169), x, depth=169)
    m = _new_model(torch.float32, "preact", 169)
    hm = m(x.cuda()).cpu()
    names = [c[0] for c in m._last_plan.prog.calls]
    err = (hm - want).abs().max().item()
    print(f"densenet169 fp32 1x64x64: max abs vs live restatement {err:.3e} on a range of {(want.max() - want.min()).item():.2f}")
    assert names.count("ft_preact_conv1x1_fwd") == 82 + 3 + 1 and m.planes == [256, 512, 1280, 1664]
    assert tuple(hm.shape) == (1, 17, 16, 16) and err <= 1e-3


def test_fpn_densenet_flip_keypoint_rows(hip_lib):
    """keypoints_in_plan + flip_pairs, B = 2: forward_keypoint_rows equals flip_ref.py's merge (average, left / right swap, key
    points) of two plain forwards at the flip plan's batch, bit for bit (the form of test_fpn_flip_keypoint_rows)."""
    shape = SHAPES[1][1:]
    B = 2
    x = synth.pose_crops(SEED, B, *shape)
    perm = flip_ref.perm_from_pairs(flip_ref.COCO_PAIRS, 17)
    m = _new_model(torch.float32)
    m.flip_pairs, m.keypoints_in_plan = flip_ref.COCO_PAIRS, True
    rows = m.forward_keypoint_rows(x.cuda())
    plan = m._last_plan
    names = [c[0] for c in plan.prog.calls]
    assert names[0] == "ft_hflip_nchw_f32" and names[-1] == "ft_heatmap_flip_merge" and names.count("ft_preact_conv1x1_fwd") == N_PREACT
    assert rows.data_ptr() == plan.kp_rows.data_ptr() and tuple(rows.shape) == (B, 17, 3)
    rows, idx, merged = rows.cpu(), plan.kp_idx.cpu(), plan.heatmaps.cpu()
    m.flip_pairs = None
    xf = torch.flip(x, dims=[3])
    plain = m.forward(torch.cat((x, x)).cuda()).cpu()[:B]                   # two plain forwards at the flip plan's batch
    mirrored = m.forward(torch.cat((xf, xf)).cuda()).cpu()[B:]
    w_merged, w_idx, w_rows = flip_ref.flip_keypoints_ref(plain.numpy(), mirrored.numpy(), perm, 1)
    assert torch.equal(_bits(merged), _bits(torch.from_numpy(np.array(w_merged))))
    assert torch.equal(idx, torch.from_numpy(np.array(w_idx))) and torch.equal(_bits(rows), _bits(torch.from_numpy(np.array(w_rows))))
    own, own_f = m.forward(x.cuda()).cpu(), m.forward(xf.cuda()).cpu()
    err = max((plain - own).abs().max().item(), (mirrored - own_f).abs().max().item())
    print(f"fpn_densenet flip plan: halves vs batch-{B} forwards {err:.3e}")
    assert err <= 1e-3


def test_pose_tool_runs_fpn_densenet(hip_lib):
    """tools/pose/main.main(model='fpn', backbone='densenet121') — the reference's own default configuration — routes to
    models.fpn_densenet and runs its synthetic validate."""
    from tools.pose import main as pose_main
    from tools.pose.config import opt
    saved = dict(opt.__dict__)
    try:
        out = pose_main.main(model="fpn", backbone="densenet121", num_samples=1, test_batch_size=1, input_res=(64, 64), flip_test=True)
    finally:
        opt.__dict__.clear()
        opt.__dict__.update(saved)
    assert isinstance(out["model"], models.FpnDensenet) and out["preds"].shape == (1, 17, 2) and out["scores"].shape == (1, 17, 1)
    assert np.isfinite(out["preds"]).all() and np.isfinite(out["scores"]).all()


def test_pose_runner_takes_fpn_densenet(hip_lib):
    """tracking.PoseRunner with the DenseNet model, no special case: rows for 3 boxes, equal to pose_est's through final_preds."""
    from flowtrack.pytorch_amd.tracking import PoseRunner, pose_est
    dev = torch.device("cuda", 0)
    net = _new_model(torch.float16)
    frame = torch.from_numpy((synth.uniform01(5, "frame", (384, 512, 3)) * 255).astype(np.uint8)).to(dev)
    boxes = np.array([[30, 40, 130, 300], [200, 10, 330, 380], [400, 100, 500, 250]], dtype=np.float64)
    got = PoseRunner(net)(frame, boxes)
    want = pose_est(net, frame, boxes, max_batch=8)
    assert got.shape == want.shape == (3, 17, 3) and np.isfinite(got).all()
    assert np.abs(got[..., :2] - want[..., :2]).max() <= 1e-3 and np.array_equal(got[..., 2], want[..., 2])
