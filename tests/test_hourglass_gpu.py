"""models.hg on the GPU against the reference's recorded heat maps (tests/golden/hg_golden.npz: 8 stacks at 2 x 64x64 and 2 x 96x80, 2
stacks — chains of four blocks — at 2 x 96x80): fp32 parity of every stack and the arg-max of the last, the fused level seams
against the unfused recording bit for bit, the fp16 mode, the flip plan with key points, the pose tool and PoseRunner.

Tolerances: stack i of the fp32 mode is held to tol_i = max(1e-3, 1.2e-4 x range_i) (hourglass_ref.stack_tol: the project's fp32 bar,
1e-3 on the FPN fixture's range of 9.0, carried over to the hourglass's ranges of 2e2 .. 3e3).  The hourglass's maps are smooth, so
near-ties between neighbouring pixels are common: the arg-max must be the fixture's on every live map whose fixture margin is >= 2
tol, and every other difference must be explained by a margin <= 2 x the measured error."""
import functools
import os

import numpy as np
import pytest
import torch

import flip_ref
import hourglass_ref
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.pose import models
from oracle import keypoints_ref

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "hg_golden.npz"), allow_pickle=False)
SEED = int(G["seed"])
CONFIGS = [tuple(int(v) for v in c) for c in G["configs"]]            # (8, 2, 64, 64), (8, 2, 96, 80), (2, 2, 96, 80)
CONFIG_IDS = ["s%d_b%d_%dx%d" % c for c in CONFIGS]
#: fp16 against the fp32 fixture, 8 stacks at 2 x 96x80, largest max-abs error / range over the stacks: measured 1.63e-3 on an MI355X
#: (stack 4; the last stack 1.37e-3); the guard is 2 x that, rounded up to one digit (test_hg_fp16_vs_fp32_fixture)
FP16_REL_GUARD = 4e-3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tag(cfg):
    return "s%d_b%d_%dx%d" % cfg


@functools.lru_cache(maxsize=None)
def _state_dict(S):
    return synth.fill_hg_state_dict(models.hg(17, S).state_dict(), SEED)


def _new_model(S, dtype, fuse=True):
    m = models.hg(num_classes=17, num_stacks=S)
    m.load_state_dict(_state_dict(S))
    m = m.cuda().eval()
    m.compute_dtype, m.fuse_seams = dtype, fuse
    return m


@functools.lru_cache(maxsize=None)
def _model(S, dtype, fuse=True):
    return _new_model(S, dtype, fuse)


def _names(m):
    return [c[0] for c in m._last_plan.prog.calls]


def _check_argmax(hm_last, cfg, err, tol=None):
    """The last stack's arg-max against the fixture's: identical on every live map with a margin >= 2 tol (where a tol is given);
    every difference explained by a margin <= 2 err."""
    tag = _tag(cfg)
    _, _, idx = keypoints_ref.max_preds_ref(hm_last.numpy())
    same = idx == G[tag + "_idx"]
    margin = G[tag + "_margin"][-1]
    live = G[tag + "_scores"][..., 0] > 0
    if tol is not None:
        firm = live & (margin >= 2 * tol)
        assert firm.sum() >= 0.75 * live.sum() > 0
        assert same[firm].all(), "arg-max differs from the reference's on a live map whose margin is >= 2 tol"
    assert np.all(margin[~same] <= 2 * err + 1e-6), "an arg-max difference that is not explained by a near-tie"
    return same


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_hg_fp32_parity(hip_lib, cfg):
    S, B, H, W = cfg
    tag = _tag(cfg)
    x = synth.pose_crops(SEED, B, H, W).cuda()
    m = _model(S, torch.float32)
    out = m(x)
    gold = torch.from_numpy(G[tag + "_heatmaps"])
    assert isinstance(out, list) and len(out) == S and all(tuple(t.shape) == (B, 17, H // 4, W // 4) and t.dtype == torch.float32 for t in out)
    errs = []
    for i, t in enumerate(out):
        rng = float(gold[i].max() - gold[i].min())
        err = (t.cpu() - gold[i]).abs().max().item()
        errs.append(err)
        print(f"hg fp32 {tag} stack {i}: max abs {err:.3e} on a range of {rng:.1f} = {err / rng:.2e}, tol {hourglass_ref.stack_tol(rng):.3e}")
        assert err <= hourglass_ref.stack_tol(rng), f"stack {i}: {err:.3e} > {hourglass_ref.stack_tol(rng):.3e}"
    last = gold[-1]
    same = _check_argmax(out[-1].cpu(), cfg, errs[-1], hourglass_ref.stack_tol(float(last.max() - last.min())))
    print(f"hg fp32 {tag}: arg-max identical on {same.mean():.4f} of the maps")
    plan = m._last_plan
    names = _names(m)
    assert names.count("ft_hourglass_down_fwd") == 4 * S + 1 and names.count("ft_hourglass_up_fwd") == 4 * S
    assert plan.heatmaps.data_ptr() == plan.stages[f"heatmap.{S - 1}"].data_ptr()
    again = m(x)                                         # the captured graph
    assert plan.runs >= 2 and plan.prog.graph_exec is not None
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, out))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_hg_fused_seams_are_bit_identical(hip_lib, dtype):
    """fuse_seams = False records pool alone, sum alone and stand-alone activations; True writes the activated copies at the seams.
    Same arithmetic, same rounding points: every stack's heat maps are bit-identical.  8 stacks at 2 x 64x64."""
    cfg = CONFIGS[0]
    S, B, H, W = cfg
    x = synth.pose_crops(SEED, B, H, W).cuda()
    fused, plain = _model(S, dtype, True), _model(S, dtype, False)
    a, b = fused(x), plain(x)
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))
    nf, npl = _names(fused), _names(plain)
    for names in (nf, npl):     # per stack 4 levels, each one down and one up; one more down behind res1
        assert names.count("ft_hourglass_down_fwd") == 4 * S + 1 and names.count("ft_hourglass_up_fwd") == 4 * S
    # one block per chain: stand-alone activations remain in front of hg[0][3], the lowest hg[0][2] (per stack) and res3
    assert nf.count("ft_scale_shift_act_nhwc_fwd") == 2 * S + 1
    # unfused: two more per level's way down (one behind res1), one more per way up
    assert npl.count("ft_scale_shift_act_nhwc_fwd") == 2 * S + 1 + (8 * S + 1) + 4 * S
    assert len(nf) < len(npl)


def test_hg_fp16_vs_fp32_fixture(hip_lib):
    """fp16 at 8 stacks, 2 x 96x80, against the fp32 fixture.  The bar cannot be derived (112 blocks deep): it is 2 x the ratio
    measured on an MI355X, rounded up to one digit — the factor 2 is the project's own for box-to-box spread, as for
    exact_argmax_rel_bound.  Every arg-max flip must be explained by a fixture margin <= 2 x the error.
    Measured on an MI355X, per stack 0..7, max abs / range: 5.7e-4, 6.0e-4, 9.2e-4, 1.10e-3, 1.63e-3, 1.20e-3, 9.5e-4, 1.37e-3 (4.1 on a
    range of 3015); worst 1.63e-3 -> guard 4e-3 (FP16_REL_GUARD); arg-max identical on all 34 maps."""
    cfg = CONFIGS[1]
    S, B, H, W = cfg
    tag = _tag(cfg)
    x = synth.pose_crops(SEED, B, H, W).cuda()
    m = _model(S, torch.float16)
    out = [t.cpu() for t in m(x)]
    gold = torch.from_numpy(G[tag + "_heatmaps"])
    worst, last_err = 0.0, 0.0
    for i, t in enumerate(out):
        rng = float(gold[i].max() - gold[i].min())
        last_err = (t - gold[i]).abs().max().item()
        worst = max(worst, last_err / rng)
        print(f"hg fp16 {tag} stack {i}: max abs {last_err:.3e} on a range of {rng:.1f} = {last_err / rng:.3e} of the range")
    same = _check_argmax(out[-1], cfg, last_err)
    print(f"hg fp16 {tag}: worst ratio {worst:.3e} = {worst / FP16_REL_GUARD:.3f} of the guard; arg-max identical {same.mean():.4f}")
    assert all(torch.isfinite(t).all() for t in out)
    assert worst <= FP16_REL_GUARD, f"fp16 heat-map error {worst:.3e} of the range"
    assert all(torch.equal(_bits(a.cpu()), _bits(b)) for a, b in zip(m(x), out))


def test_hg_flip_keypoint_rows(hip_lib):
    """keypoints_in_plan + flip_pairs on an hourglass, B = 2 at 64x64 (the form of test_fpn_flip_keypoint_rows): the rows of the flip
    plan equal flip_ref.py's merge of the model's own batch-2B last-stack maps, bit for bit."""
    S, B, H, W = 2, 2, 64, 64
    x = synth.pose_crops(SEED, B, H, W)
    perm = flip_ref.perm_from_pairs(flip_ref.COCO_PAIRS, 17)
    m = _new_model(S, torch.float32)
    m.flip_pairs, m.keypoints_in_plan = flip_ref.COCO_PAIRS, True
    rows = m.forward_keypoint_rows(x.cuda())
    plan = m._last_plan
    names = _names(m)
    assert names[0] == "ft_hflip_nchw_f32" and names[-1] == "ft_heatmap_flip_merge" and names.count("ft_hourglass_up_fwd") == 4 * S
    assert rows.data_ptr() == plan.kp_rows.data_ptr() and tuple(rows.shape) == (B, 17, 3)
    rows, idx, merged = rows.cpu(), plan.kp_idx.cpu(), plan.heatmaps.cpu()
    m.flip_pairs = None
    xf = torch.flip(x, dims=[3])
    plain = m.forward(torch.cat((x, x)).cuda())[-1].cpu()[:B]                # two plain forwards at the flip plan's batch
    mirrored = m.forward(torch.cat((xf, xf)).cuda())[-1].cpu()[B:]
    w_merged, w_idx, w_rows = flip_ref.flip_keypoints_ref(plain.numpy(), mirrored.numpy(), perm, 1)
    assert torch.equal(_bits(merged), _bits(torch.from_numpy(np.array(w_merged))))
    assert torch.equal(idx, torch.from_numpy(np.array(w_idx))) and torch.equal(_bits(rows), _bits(torch.from_numpy(np.array(w_rows))))
    # forward_flip returns the same merged map (a tensor: the flip test is built on the last stack)
    m.flip_pairs = flip_ref.COCO_PAIRS
    assert torch.equal(_bits(m.forward_flip(x.cuda()).cpu()), _bits(merged))


def test_pose_tool_runs_hg(hip_lib):
    """tools/pose/main.main(model='hg') builds models.hg(num_classes, num_stacks=8) as the reference does and runs its synthetic
    validate with the flip test; model='pose' is still refused."""
    from tools.pose import main as pose_main
    from tools.pose.config import opt
    saved = dict(opt.__dict__)
    try:
        out = pose_main.main(model="hg", num_samples=1, test_batch_size=1, input_res=(64, 64), flip_test=True)
        name = opt.model_name
    finally:
        opt.__dict__.clear()
        opt.__dict__.update(saved)
    assert isinstance(out["model"], models.HourglassNet) and out["model"].num_stacks == 8 and name == "hg"
    assert out["preds"].shape == (1, 17, 2) and out["scores"].shape == (1, 17, 1)
    assert np.isfinite(out["preds"]).all() and np.isfinite(out["scores"]).all()
    with pytest.raises(ValueError, match="deconv.*fpn"):
        pose_main.main(model="pose", backbone="resnet50")
    opt.__dict__.clear()
    opt.__dict__.update(saved)


def test_pose_runner_takes_hg(hip_lib):
    """tracking.PoseRunner with an hourglass, no special case: finite rows for 3 boxes from a plan that holds the hourglass's
    launches, the same again on the second call (the captured graph)."""
    from flowtrack.pytorch_amd.tracking import PoseRunner
    dev = torch.device("cuda", 0)
    net = _new_model(2, torch.float32)
    frame = torch.from_numpy((synth.uniform01(5, "frame", (384, 512, 3)) * 255).astype(np.uint8)).to(dev)
    boxes = np.array([[30, 40, 130, 300], [200, 10, 330, 380], [400, 100, 500, 250]], dtype=np.float64)
    runner = PoseRunner(net, inp_res=(64, 64))
    got = runner(frame, boxes)
    assert got.shape == (3, 17, 3) and np.isfinite(got).all()
    assert any(c[0] == "ft_hourglass_down_fwd" for pl in net._plans.values() for c in pl.prog.calls)
    assert np.array_equal(runner(frame, boxes), got)
