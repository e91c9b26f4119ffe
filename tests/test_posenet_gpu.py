"""models.pose on the GPU against the reference's recorded heat maps (tests/golden/posenet_golden.npz) and the live CPU restatement
(tests/posenet_ref.py::posenet_forward): fp32 parity and integer-exact arg-max at both golden shapes, with the first-call benchmark's
pick and with each form of the top-down steps forced ("kconcat": one launch per step, "lateral+deconv": two), the fp16 mode in the form
of test_fpn_fp16_vs_fp32_reference, full stage seams whatever FT_FUSE_STAGE_EXIT says, the flip plan, PoseRunner, the device tracking
pass and the demo's model construction.

Measured on an MI355X: fp32 max abs against the fixture 7.6e-06 (2 x 128x96) and 6.2e-06 (3 x 64x64) with the benchmark's pick, 8.1e-06 /
6.7e-06 with "kconcat" forced, 7.6e-06 / 6.2e-06 with "lateral+deconv" forced, scores 3.8e-06, smallest margin of a map with score > 0
1.4e-02 / 1.4e-02, the two forced forms 5.7e-06 apart; fp16 at 2 x 128x96 9.1e-03 on a range of 13.1 = 0.69e-3 of the range = 0.23 of the
3e-3 guard (kconcat 0.22, lateral+deconv 0.20; under a quarter of it: the guard stays), arg-max identical on every map; the two forced
forms in fp16 4.6e-03 apart (0.35e-3 of the range).  A second session (other tile picks): fp16 0.21 / 0.21 / 0.20 of the guard, the forms
5.3e-03 apart."""
import functools
import os

import numpy as np
import pytest
import torch

import flip_ref
import posenet_ref
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.pose import models
from oracle import keypoints_ref

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "posenet_golden.npz"), allow_pickle=False)
SEED = int(G["seed"])
SHAPES = [tuple(int(v) for v in s) for s in G["shapes"]]            # (2, 128, 96), (3, 64, 64)
SHAPE_IDS = ["x".join(str(v) for v in s) for s in SHAPES]
FORMS = models.LateralDeconvResnet.STEP_FORMS                       # "kconcat", "lateral+deconv"
STAGES = ("layer1", "layer2", "layer3", "layer4", "a5", "a4", "a3", "a2")


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _state_dict():
    return synth.fill_pose_state_dict(models.pose("resnet50", num_classes=17, pretrained=False).state_dict(), SEED)


def _new_model(dtype, form=None):
    m = models.pose("resnet50", num_classes=17, pretrained=False)
    m.load_state_dict(_state_dict())
    m = m.cuda().eval()
    m.compute_dtype = dtype
    m.lateral_step_form = form
    return m


@functools.lru_cache(maxsize=None)
def _model(dtype, form=None):
    return _new_model(dtype, form)


@functools.lru_cache(maxsize=None)
def _live(shape):
    """(x, posenet_forward(x)) on the CPU, once per shape."""
    x = synth.pose_crops(SEED, *shape)
    return x, posenet_ref.posenet_forward(_state_dict(), x, depth=50)


def _tag(shape):
    return "b%d_%dx%d" % shape


def _names(plan):
    return [c[0] for c in plan.prog.calls]


def _step_launches(plan):
    """Per top-down step, the labels of its conv launches in the resolved plan."""
    recs = [r[0] for r in plan.prog.conv_records]
    return [[l for l in recs if l.startswith((f"deconv{j}.2", f"latlayer{j + 1}"))] for j in (1, 2, 3)]


def _check_launch_list(plan, form=None):
    names = _names(plan)
    assert names.count("ft_scale_shift_act_nhwc_fwd") == 1 and not any(n.startswith("ft_bottleneck_exit") for n in names)
    assert not any(n.startswith("__") for n in names), "an unresolved choice in a plan that ran"
    for stage in STAGES:
        assert stage in plan.stages
    for j, labels in enumerate(_step_launches(plan), start=1):
        one, two = [f"deconv{j}.2+latlayer{j + 1}"], [f"latlayer{j + 1}.bn", f"deconv{j}.2+residual"]
        assert labels in ((one,) if form == "kconcat" else (two,) if form == "lateral+deconv" else (one, two)), labels


def _check_fp32(hm, shape, what):
    """<= 1e-3 max-abs against the fixture and the live restatement; arg-max integer-exact on every map with score > 0, scores <= 1e-3."""
    tag = _tag(shape)
    gold = torch.from_numpy(G[tag + "_heatmaps"])
    err_gold = (hm - gold).abs().max().item()
    err_live = (hm - _live(shape)[1]).abs().max().item()
    _, scores, idx = keypoints_ref.max_preds_ref(hm.numpy())
    live = G[tag + "_scores"][..., 0] > 0
    err_score = np.abs(scores - G[tag + "_scores"]).max()
    print(f"{what} {tag}: max abs vs fixture {err_gold:.3e}, vs live posenet_forward {err_live:.3e}, scores {err_score:.3e}, "
          f"{int(live.sum())} live maps, smallest live margin {G[tag + '_margin'][live].min():.3e}")
    assert tuple(hm.shape) == tuple(gold.shape)
    assert err_gold <= 1e-3 and err_live <= 1e-3 and err_score <= 1e-3
    assert np.array_equal(idx[live], G[tag + "_idx"][live]), "arg-max differs from the reference's on a map with score > 0"


@pytest.mark.parametrize("form", [None] + list(FORMS), ids=["benchmarked", "kconcat", "lateral_deconv"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_posenet_fp32_parity(hip_lib, shape, form):
    x, _ = _live(shape)
    m = _model(torch.float32, form)
    hm = m(x.cuda())
    _check_fp32(hm.cpu(), shape, f"fp32 {form or 'benchmarked'}")
    plan = m._last_plan
    _check_launch_list(plan, form)
    again = m(x.cuda())                                  # the captured graph
    assert plan.runs >= 2 and plan.prog.graph_exec is not None and torch.equal(_bits(again), _bits(hm))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_forced_forms_agree(hip_lib, shape, dtype):
    """fp32: the two forms agree to the fp32 bar, 1e-3.  fp16: the two-launch form stores l = s lat(c) + b in fp16 between its launches,
    a rounding the one-launch form does not have (half an fp16 ulp of a value of the heat maps' own size, per step), so the forms are
    two different fp16 evaluations; each is held to the fp16 guard of 3e-3 of the reference's range against the fp32 reference
    (test_posenet_fp16_vs_fp32_reference), so they can differ by at most twice the guard, and that is what is asserted here."""
    x, want = _live(shape)
    a, b = (_model(dtype, f)(x.cuda()).cpu() for f in FORMS)
    err = (a - b).abs().max().item()
    rng = (want.max() - want.min()).item()
    print(f"{_tag(shape)} {dtype}: kconcat vs lateral+deconv {err:.3e} (range {rng:.3f}: {err / rng:.3e} of it)")
    assert err <= (1e-3 if dtype == torch.float32 else 2 * 3e-3 * rng)


def test_unknown_form_is_refused(hip_lib):
    from flowtrack.pytorch_amd._lib import FlowtrackHipError
    m = _new_model(torch.float32, "fused")
    with pytest.raises(FlowtrackHipError, match="lateral_step_form"):
        m(torch.zeros(1, 3, 64, 64).cuda())


@pytest.mark.parametrize("form", [None] + list(FORMS), ids=["benchmarked", "kconcat", "lateral_deconv"])
def test_posenet_fp16_vs_fp32_reference(hip_lib, form):
    """The form of test_fpn_fp16_vs_fp32_reference at 2 x 128x96: max-abs error against the fp32 CPU reference <= 3e-3 of the
    heat-map range (the project's guard for the fp16 mode), >= 97 % identical arg-max, every mismatch a near-tie (margin <= 2 err),
    a repeat gives equal bits."""
    shape = SHAPES[0]
    x, want = _live(shape)
    tag = _tag(shape)
    m = _model(torch.float16, form)
    hm = m(x.cuda()).cpu()
    err = (hm - want).abs().max().item()
    rng = (want.max() - want.min()).item()
    _, _, idx = keypoints_ref.max_preds_ref(hm.numpy())
    same = idx == G[tag + "_idx"]
    print(f"posenet fp16 {form or 'benchmarked'} {tag}: max abs {err:.3e} on a range of {rng:.3f} = {err / rng:.3e} of the range = "
          f"{err / (3e-3 * rng):.3f} of the guard; arg-max identical {same.mean():.4f}")
    assert err <= 3e-3 * rng, f"fp16 heatmap error {err:.3e} vs range {rng:.2f}"
    assert same.mean() >= 0.97, f"only {same.mean():.3f} of arg-max indices match"
    assert np.all(G[tag + "_margin"][~same] <= 2 * err + 1e-6), "an arg-max flip that is not explained by a near-tie"
    assert torch.equal(_bits(m(x.cuda()).cpu()), _bits(hm))
    _check_launch_list(m._last_plan, form)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_posenet_ignores_forced_stage_exit(hip_lib, monkeypatch, dtype):
    """The exit form writes only the even pixels of a stage's last block, and this head reads the full maps of layer1 .. layer3: with
    the exit form forced the plan still records every seam in full and gives the plain model's result."""
    monkeypatch.setenv("FT_FUSE_STAGE_EXIT", "2")
    shape = SHAPES[0]
    x, _ = _live(shape)
    m = _new_model(dtype)
    m.fuse_stage_exit = "force"
    hm = m(x.cuda()).cpu()
    plan = m._last_plan
    assert not any(c[0].startswith("ft_bottleneck_exit") for c in plan.prog.calls) and not plan.stages.absent
    for li, c in ((1, 256), (2, 512), (3, 1024)):
        v = plan.stages[f"layer{li}"]
        assert (v.H, v.W, v.C) == (shape[1] // (2 << li), shape[2] // (2 << li), c)
    for j, name in enumerate(("a5", "a4", "a3", "a2")):
        v = plan.stages[name]
        assert (v.H, v.W, v.C) == ((shape[1] // 32) << j, (shape[2] // 32) << j, 2048 if j == 0 else 256)
    if dtype == torch.float32:
        _check_fp32(hm, shape, "forced stage exit")
    want = _model(dtype)(x.cuda()).cpu()
    assert (hm - want).abs().max().item() <= 1e-3


def test_posenet_flip_keypoint_rows(hip_lib):
    """keypoints_in_plan + flip_pairs, B = 2, built as test_fpn_flip_keypoint_rows builds it: forward_keypoint_rows equals flip_ref.py's
    merge (average, left / right swap, key points) of two plain forwards run at the flip plan's batch, bit for bit; against two
    batch-B forwards the halves are held to the fp32 bar.  One form is forced, so that the batch-2B and batch-B plans cannot differ
    in the benchmark's pick."""
    shape = SHAPES[1][1:]
    B = 2
    x = synth.pose_crops(SEED, B, *shape)
    perm = flip_ref.perm_from_pairs(flip_ref.COCO_PAIRS, 17)
    m = _new_model(torch.float32, "kconcat")
    m.flip_pairs, m.keypoints_in_plan = flip_ref.COCO_PAIRS, True
    rows = m.forward_keypoint_rows(x.cuda())
    plan = m._last_plan
    names = _names(plan)
    assert names[0] == "ft_hflip_nchw_f32" and names[-1] == "ft_heatmap_flip_merge" and names.count("ft_scale_shift_act_nhwc_fwd") == 1
    assert rows.data_ptr() == plan.kp_rows.data_ptr() and tuple(rows.shape) == (B, 17, 3)
    rows, idx, merged = rows.cpu(), plan.kp_idx.cpu(), plan.heatmaps.cpu()
    assert torch.equal(_bits(m.forward_flip(x.cuda()).cpu()), _bits(merged)) and m._last_plan is plan      # forward_flip: the same plan's merged maps
    m.flip_pairs = None
    xf = torch.flip(x, dims=[3])
    plain = m.forward(torch.cat((x, x)).cuda()).cpu()[:B]                   # two plain forwards at the flip plan's batch
    mirrored = m.forward(torch.cat((xf, xf)).cuda()).cpu()[B:]
    w_merged, w_idx, w_rows = flip_ref.flip_keypoints_ref(plain.numpy(), mirrored.numpy(), perm, 1)
    assert torch.equal(_bits(merged), _bits(torch.from_numpy(np.array(w_merged))))
    assert torch.equal(idx, torch.from_numpy(np.array(w_idx))) and torch.equal(_bits(rows), _bits(torch.from_numpy(np.array(w_rows))))
    own, own_f = m.forward(x.cuda()).cpu(), m.forward(xf.cuda()).cpu()
    err = max((plain - own).abs().max().item(), (mirrored - own_f).abs().max().item())
    print(f"posenet flip plan: halves vs batch-{B} forwards {err:.3e}")
    assert err <= 1e-3


def test_pose_runner_takes_posenet(hip_lib):
    """tracking.PoseRunner with a lateral-deconv model, no special case: rows for 3 boxes, equal to pose_est's through final_preds."""
    from flowtrack.pytorch_amd.tracking import PoseRunner, pose_est
    dev = torch.device("cuda", 0)
    net = _new_model(torch.float16)
    frame = torch.from_numpy((synth.uniform01(5, "frame", (384, 512, 3)) * 255).astype(np.uint8)).to(dev)
    boxes = np.array([[30, 40, 130, 300], [200, 10, 330, 380], [400, 100, 500, 250]], dtype=np.float64)
    got = PoseRunner(net)(frame, boxes)
    want = pose_est(net, frame, boxes, max_batch=8)
    assert got.shape == want.shape == (3, 17, 3) and np.isfinite(got).all()
    assert np.abs(got[..., :2] - want[..., :2]).max() <= 1e-3 and np.array_equal(got[..., 2], want[..., 2])


def test_demo_builds_posenet_and_device_pass_takes_it(hip_lib):
    """tools/tracking/demo.py's model construction with pose_head='pose' builds a LateralDeconvResnet, and DeviceTrackingPass runs a
    clip with it as test_device_pass_replays_as_the_host_pass runs one with the deconv model: the host pass, answered with the rows
    the device pass placed, asks for the same boxes and ends with the same boxes, key points and ids."""
    import types
    from flowtrack.pytorch_amd.tracking import DeviceTrackingPass, PoseRunner
    from tools.tracking import demo
    dev = torch.device("cuda:0")
    args = types.SimpleNamespace(pose_backbone=50, pose_head="pose", pose_model="", flow_net="FlowNet2S", flow_model="", fp16=True)
    pose_net, flow_net = demo.build_nets(args, dev)
    assert isinstance(pose_net, models.LateralDeconvResnet) and pose_net.compute_dtype == torch.float16
    T = 4
    frames, dets = demo.synthetic_clip(T, H=192, W=256, n_people=3, seed=4)
    runner = PoseRunner(pose_net)
    fr, flows, kp_all, _ = demo._batched_phases(frames, dets, pose_net, flow_net, 0, 1, 16, T, None, flow_net, dev, runner, on_device=True)
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
    want = demo.tracking_pass(dets, [kp_host[t, :len(dets[t])] for t in range(T)], flows.cpu().numpy(), pose_boxes, 0.3, "2x")
    assert len(got) == len(want) == T and asked, "no propagated box survived in any frame: the replay checked nothing"
    for g, w in zip(got, want):
        assert np.array_equal(g["boxes"], w["boxes"]) and np.array_equal(g["keypoints"], w["keypoints"]) and list(g["ids"]) == list(w["ids"])
    assert np.isfinite(np.concatenate([g["keypoints"].ravel() for g in got])).all()
