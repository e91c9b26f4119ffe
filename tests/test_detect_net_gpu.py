"""detection.nets.resnetv1 / detection.test on the GPU against the reference's recorded run (tests/golden/detect_net_golden.npz):
the continuous seams in the fp32 parity mode and the fp16 mode, the discrete steps against restatements fed with the run's OWN inputs,
the fused forms against plain launches, plan reuse, and the demo tool.

Measured on an MI355X (case a / b): fp32 net_conv 1.4e-05 / 1.7e-05 on values of 15 / 16, rpn_cls_score 1.1e-05 / 1.2e-05,
rpn_bbox_pred 1.1e-06 / 1.2e-06, cls_score 2.2e-06 / 1.7e-06, bbox_pred 2.4e-07 / 4.0e-07; fp16 net_conv 2.0e-02 / 1.7e-02
(0.44 / 0.36 of the 3e-3-of-range guard), rpn_cls_prob 1.8e-03 / 1.3e-03, cls_score 1.2e-03 / 1.1e-03."""
import functools
import os

import numpy as np
import pytest
import torch

import detect_net_ref as R
import detect_ref
from conftest import GOLDEN, ROOT
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.detection import nets, test as det_test

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "detect_net_golden.npz"), allow_pickle=False)
SEED, TARGET, MAX_SIZE = int(G["seed"]), int(G["target_size"]), int(G["max_size"])
K, PERSON, A = int(G["num_classes"]), int(G["person_id"]), 9
CASES = ("a", "b")
DTYPES = [torch.float32, torch.float16]
DTYPE_IDS = ["fp32", "fp16"]
TRUNK_SEAMS = ("net_conv", "rpn_cls_score", "rpn_bbox_pred", "rpn_cls_prob")
HEAD_SEAMS = ("cls_score", "bbox_pred", "cls_prob")


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _state_dict():
    net = nets.resnetv1(50)
    net.create_architecture(K, tag="default")
    return synth.fill_detector_state_dict(net.state_dict(), SEED)


def _new_net(dtype):
    net = nets.resnetv1(50)
    net.create_architecture(K, tag="default")
    net.load_state_dict(_state_dict())
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


@functools.lru_cache(maxsize=None)
def _net(dtype):
    return _new_net(dtype)


def _frame(case):
    h, w = (int(v) for v in G[case + "_frame_hw"])
    return synth.detector_frame(SEED, h, w)


def _run(net, case, keep=True):
    """im_detect's steps with every seam kept: the predictions as numpy."""
    plan, im_info, _, shape = det_test.stage_frame(net, _frame(case), TARGET, MAX_SIZE)
    p = net.detect_staged(plan, im_info, frame_shape=shape, keep_intermediates=keep)
    return plan, im_info, shape, {k: v.cpu().numpy() for k, v in p.items()}


def _tolerance(dtype, name, gold):
    if dtype == torch.float32:
        return 1e-3 if name.endswith("_prob") else 1e-3 * max(1.0, float(np.abs(gold).max()))      # the project's fp32 bar
    return 3e-3 * float(gold.max() - gold.min())                                                   # the fp16 guard: 3e-3 of the range


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_continuous_seams(hip_lib, dtype, case):
    net = _net(dtype)
    plan, im_info, shape, p = _run(net, case)
    assert np.array_equal(im_info, G[case + "_im_info"])
    assert np.abs(plan.x_static.cpu().numpy() - G[case + "_blob"]).max() <= R.blob_bound(_frame(case), R.PIXEL_MEANS) + 2e-5
    head = net.region_head(plan, torch.from_numpy(G[case + "_rois"]).cuda(), float(im_info[2]), shape, keep_intermediates=True)
    p.update({k: head[k].cpu().numpy() for k in HEAD_SEAMS + ("pool5", "fc7")})      # the region head on the GOLDEN's rois
    for name in TRUNK_SEAMS + HEAD_SEAMS:
        gold = G[f"{case}_{name}"]
        assert p[name].shape == gold.shape and p[name].dtype == np.float32, name
        err, tol = float(np.abs(p[name] - gold).max()), _tolerance(dtype, name, gold)
        print(f"{DTYPE_IDS[DTYPES.index(dtype)]} case {case} {name}: max abs {err:.3e}, tolerance {tol:.3e} ({err / tol:.3f} of it)")
        assert err <= tol, (name, err, tol)
    assert p["pool5"].shape == (len(G[case + "_rois"]), 1024, 7, 7) and p["fc7"].shape == (len(G[case + "_rois"]), 2048)
    assert set(net._predictions) >= {"rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "rois", "cls_score", "cls_pred", "cls_prob", "bbox_pred"}
    assert np.array_equal(net._predictions["cls_pred"].cpu().numpy(), net._predictions["cls_score"].cpu().numpy().argmax(1))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_discrete_steps_follow_their_own_inputs(hip_lib, dtype, case):
    net = _net(dtype)
    frame = _frame(case)
    h, w = frame.shape[:2]
    _, im_info, _, p = _run(net, case, keep=False)
    # the proposal layer: decode + stable sort + NMS of the run's own RPN outputs
    fh, fw = p["rpn_cls_prob"].shape[1:3]
    anchors = R.anchors_for(fh, fw)
    blob, _, idx = detect_ref.proposal_layer(p["rpn_cls_prob"], p["rpn_bbox_pred"], im_info, anchors, A, 6000, 300, 0.7, np.float64)
    assert p["rois"].shape == blob.shape and 0 < len(blob) < len(anchors)
    bound = detect_ref.decode_bound(anchors[idx], p["rpn_bbox_pred"].reshape(-1, 4)[idx]) + 2.0 ** -23 * np.abs(blob[:, 1:])
    assert np.all(p["rois"][:, 0] == 0) and np.all(np.abs(p["rois"][:, 1:] - blob[:, 1:]) <= bound), "another order, or boxes beyond decode_bound"
    # test_image on the same blob (the reference's [1,H,W,3] layout) returns the same four arrays
    plan = net.trunk_plan(int(im_info[0]), int(im_info[1]))
    cls_score, cls_prob, bbox_pred, rois = net.test_image(plan.x_static.cpu().numpy().transpose(0, 2, 3, 1), im_info)
    assert np.array_equal(rois, p["rois"]) and np.array_equal(cls_score, p["cls_score"]) and np.array_equal(bbox_pred, p["bbox_pred"])
    # scores / pred_boxes of im_detect: the softmax and the decode of the run's own cls_score, bbox_pred and rois
    scores, pred_boxes = det_test.im_detect(net, frame, TARGET, MAX_SIZE)
    assert np.array_equal(scores, p["cls_prob"]) and np.array_equal(pred_boxes, p["pred_boxes"])
    ones, zeros = (1.0,) * 4, (0.0,) * 4              # bbox_pred is un-normalised already
    want = R.detections_ref(p["cls_score"], p["bbox_pred"], p["rois"], ones, zeros, im_info[2], h, w, np.float64)
    assert np.all(np.abs(scores - want[0]) <= R.softmax_bound(p["cls_score"], 1))
    assert np.all(np.abs(pred_boxes - want[2]) <= R.detections_bound(p["bbox_pred"], p["rois"], ones, zeros, im_info[2]))
    # the person NMS: exactly detect_ref.nms on the run's own person rows, with and without extra boxes
    extra = np.array([[5, 5, 30, 40, 0.99], [4, 6, 31, 41, 0.5], [40, 10, 60, 45, 0.2]], dtype=np.float32)
    for prop in (None, extra):
        got = det_test.detect_persons(net, frame, PERSON, 0.3, prop, target_size=TARGET, max_size=MAX_SIZE)
        want_p = R.detect_persons(scores, pred_boxes, PERSON, 0.3, prop)
        assert got.dtype == np.float32 and np.array_equal(got, want_p)
        assert 1 <= len(got) < len(scores) + (0 if prop is None else len(prop))


def test_fused_forms_against_plain_launches(hip_lib):
    """fp32 mode: the K-concatenated conv3 + shortcut GEMM folds both BatchNorms into its weights, so it is not bit-equal to the
    two launches it replaces: the plain-launch net_conv stays within the fp32 bar of the fused one (and of the golden)."""
    fused, plain = _net(torch.float32), _new_net(torch.float32)
    plain.fuse_shortcut = plain.fuse_bottleneck = False
    for case in CASES:
        pf, _, _, a = _run(fused, case)
        pp, _, _, b = _run(plain, case)
        names_f, names_p = [c[0] for c in pf.prog.calls], [c[0] for c in pp.prog.calls]
        assert len(names_p) == len(names_f) + 3 and not pf.fallbacks                 # layer1.0, layer2.0, layer3.0: one launch more each
        gold = G[case + "_net_conv"]
        tol = 1e-3 * max(1.0, float(np.abs(gold).max()))
        err = float(np.abs(a["net_conv"] - b["net_conv"]).max())
        print(f"case {case}: fused vs plain net_conv {err:.3e}, plain vs golden {np.abs(b['net_conv'] - gold).max():.3e}, tolerance {tol:.3e}")
        assert err <= tol and np.abs(b["net_conv"] - gold).max() <= tol


@pytest.mark.parametrize("case", CASES)
def test_fp16_fused_blocks_at_odd_maps(hip_lib, case):
    """Every identity block of layer1..layer3 pinned to its one-launch form (fuse_bottleneck = "force": no choice for the first-call
    benchmark to make) at the golden's odd maps, against the same net on three convs per block and against the golden: net_conv
    within the fp16 guard, 3e-3 of the golden's range, both ways."""
    forced, plain = _new_net(torch.float16), _new_net(torch.float16)
    forced.fuse_bottleneck, plain.fuse_bottleneck = "force", False
    pf, _, _, a = _run(forced, case)
    pp, _, _, b = _run(plain, case)
    names_f, names_p = [c[0] for c in pf.prog.calls], [c[0] for c in pp.prog.calls]
    fused = [n for n in names_f if n in ("ft_bottleneck_fwd", "ft_bottleneck_stream_fwd")]
    assert len(fused) == 2 + 3 + 5 and pf.fallbacks == [] and "ft_bottleneck_fwd" in fused and "ft_bottleneck_stream_fwd" in fused
    assert not any(n.startswith("ft_bottleneck") for n in names_p)
    gold = G[case + "_net_conv"]
    tol = _tolerance(torch.float16, "net_conv", gold)
    e_fp, e_fg, e_pg = (float(np.abs(x - y).max()) for x, y in ((a["net_conv"], b["net_conv"]), (a["net_conv"], gold), (b["net_conv"], gold)))
    print(f"fp16 case {case} net_conv: forced fused vs plain {e_fp:.3e}, fused vs golden {e_fg:.3e}, plain vs golden {e_pg:.3e}, guard {tol:.3e}")
    assert e_fp <= tol and e_fg <= tol and e_pg <= tol


def test_fp16_plan_structure(hip_lib):
    """The library's queries take every identity block of layer1..layer3 at the golden's odd maps (19x27, 10x14, 5x7), so the fp16
    trunk offers the one-launch form for all of them (the first-call benchmark keeps it or the three convs); the plans' glue."""
    net = _net(torch.float16)
    plan, _, _, _ = _run(net, "a")
    names = [c[0] for c in plan.prog.calls]
    assert plan.fallbacks == []
    assert names.count("ft_rpn_softmax_fwd") == 1 and names.count("ft_maxpool3x3s2_fwd") == 1 and names[0] == "ft_pack_nchw_to_nhwc"
    head = next(iter(plan.heads.values()))
    hnames = [c[0] for c in head.prog.calls]
    assert hnames[0] == "ft_roi_crop_nhwc_fwd" and hnames.count("ft_rcnn_mean_pool_fwd") == 1 and head.rois.shape == (300, 5)


def test_even_maps_get_no_form_the_detector_does_not_offer(hip_lib):
    """A 128x192 blob has even maps throughout (32x48, 16x24, 8x12), where the library's queries would also take the pose trunk's
    entry / head forms (layer1.0 is 64 -> 64 -> 256 at stride 1): the shared block recorder must offer the detector only whole
    identity blocks and the shortcut GEMM.  The plan is built, not run."""
    from flowtrack.pytorch_amd import _lib
    plan = _net(torch.float16).trunk_plan(128, 192)
    descs = [c[1][0]._obj for c in plan.prog.calls if c[0].startswith("ft_bottleneck")]
    assert len(descs) == 2 + 3 + 5 and all(isinstance(d, _lib.BottleneckDesc) and d.head_only == 0 and d.projection == 0 for d in descs)
    keys = [c[1][0] for c in plan.prog.calls if c[0] == "__choice__"]
    assert sum(k.startswith("bottleneck|") for k in keys) == 10 and not any(k.startswith(("entry|", "head2|", "bottleneck|exit")) for k in keys)
    assert plan.fallbacks == [] and plan.runs == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_plan_reuse_and_call_order(hip_lib, dtype):
    net = _new_net(dtype)
    plan_a, _, _, a1 = _run(net, "a", keep=False)
    assert len(net._plans) == 1 and plan_a.runs == 1 and plan_a.prog.graph_exec is not None
    other = np.ascontiguousarray(_frame("a")[::-1, ::-1])                         # another image of the same blob shape
    plan_o, im_info, _, shape = det_test.stage_frame(net, other, TARGET, MAX_SIZE)
    o = net.detect_staged(plan_o, im_info, frame_shape=shape)
    assert plan_o is plan_a and len(net._plans) == 1 and plan_a.runs == 2 and len(plan_a.heads) == 1      # replayed, not rebuilt
    assert next(iter(plan_a.heads.values())).runs == 2
    assert not np.array_equal(o["cls_score"].cpu().numpy(), a1["cls_score"])
    plan_b, _, _, b1 = _run(net, "b", keep=False)
    assert plan_b is not plan_a and len(net._plans) == 2
    _, _, _, a2 = _run(net, "a", keep=False)
    _, _, _, b2 = _run(net, "b", keep=False)
    for first, again in ((a1, a2), (b1, b2)):
        for k in ("rois", "cls_score", "cls_prob", "bbox_pred", "pred_boxes", "rpn_cls_prob"):
            assert np.array_equal(first[k].view(np.int32), again[k].view(np.int32)), k
    fresh = _new_net(dtype)                                                        # b first on a fresh model: the same bits
    _, _, _, b0 = _run(fresh, "b", keep=False)
    assert np.array_equal(b0["cls_score"].view(np.int32), b1["cls_score"].view(np.int32)) and np.array_equal(b0["rois"], b1["rois"])
    head = net.extract_head(R.blob_ref(_frame("b"), R.PIXEL_MEANS, 52, 125, 96 / 125, 96 / 125, np.float32).transpose(0, 2, 3, 1))
    assert tuple(head.shape) == (1, 1024, 4, 8) and head.dtype == torch.float32


def test_demo_tool(hip_lib, tmp_path, capsys):
    import sys
    sys.path.insert(0, ROOT)
    from tools.detection import demo
    frame = synth.detector_frame(SEED, 50, 72)
    path = tmp_path / "frame.ppm"
    path.write_bytes(b"P6\n72 50\n255\n" + np.ascontiguousarray(frame[:, :, ::-1]).tobytes())          # PPM is RGB
    assert np.array_equal(demo.load_image_bgr(str(path)), frame)
    dets = demo.main(["--net", "res50", "--num_classes", "3", "--person_id", "1", "--image", str(path), "--target_size", "75",
                      "--max_size", "125", "--seed", str(SEED)])
    out = capsys.readouterr().out
    assert dets.ndim == 2 and dets.shape[1] == 5 and np.isfinite(dets).all() and f"{len(dets)} person boxes" in out
    want = det_test.detect_persons(_net(torch.float32), frame, PERSON, 0.3, target_size=TARGET, max_size=MAX_SIZE)
    assert np.array_equal(dets, want)
