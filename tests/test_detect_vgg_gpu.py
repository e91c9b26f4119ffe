"""detection.nets.vgg16 / detection.test on the GPU against the reference's recorded run (tests/golden/detect_vgg_golden.npz): the
continuous seams in the fp32 parity mode and the fp16 mode, the discrete steps against restatements fed with the run's OWN inputs,
the two recorded forms of the classifier layers against each other, plan reuse, and the demo tool.

The bars are the project's, as tests/test_detect_net_gpu.py sets them: fp32 1e-3 * max(1, max |golden|) and 1e-3 on probabilities;
fp16 3e-3 of the golden's range.  Every test prints its errors and their share of the bar.

Measured on an MI355X (case a / b where both were read): fp32 net_conv 3.9e-05 (b) on values of 14, rpn_cls_score 1.7e-05, fc7
3.8e-06, cls_score 5.2e-06; fp16 net_conv 1.9e-02 / 1.8e-02 (0.39 / 0.42 of the guard), rpn_cls_prob 2.2e-03 / 2.3e-03 (0.72 / 0.77),
fc7 2.0e-03 / 2.1e-03 (0.30); each pinned FC form 0.089 of the two-layer bound, "fc" against "igemm" 9.8e-04 (0.022 of the allowance)."""
import functools
import os

import numpy as np
import pytest
import torch

import detect_net_ref as R
import detect_ref
import detect_vgg_ref as V
from conftest import GOLDEN, ROOT
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd.detection import nets, test as det_test

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "detect_vgg_golden.npz"), allow_pickle=False)
SEED, TARGET, MAX_SIZE = int(G["seed"]), int(G["target_size"]), int(G["max_size"])
K, PERSON, A, FC7_ROWS = int(G["num_classes"]), int(G["person_id"]), 9, int(G["fc7_rows"])
CASES = ("a", "b")
DTYPES = [torch.float32, torch.float16]
DTYPE_IDS = ["fp32", "fp16"]
TRUNK_SEAMS = ("net_conv", "rpn_cls_score", "rpn_bbox_pred", "rpn_cls_prob")
HEAD_SEAMS = ("fc7", "cls_score", "bbox_pred", "cls_prob")


@functools.lru_cache(maxsize=None)
def _state_dict():
    net = nets.vgg16()
    net.create_architecture(K, tag="default")
    return synth.fill_vgg_detector_state_dict(net.state_dict(), SEED)


@functools.lru_cache(maxsize=None)
def _net(dtype, fc_form=""):
    net = nets.vgg16()
    net.create_architecture(K, tag="default")
    net.load_state_dict(_state_dict())
    net = net.cuda().eval()
    net.compute_dtype, net.fc_form = dtype, fc_form
    return net


def _frame(case):
    h, w = (int(v) for v in G[case + "_frame_hw"])
    return synth.detector_frame(SEED, h, w)


def _run(net, case, keep=True):
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
    n = len(G[case + "_rois"])
    head = net.region_head(plan, torch.from_numpy(G[case + "_rois"]).cuda(), float(im_info[2]), shape, keep_intermediates=True)
    p.update({k: head[k].cpu().numpy() for k in HEAD_SEAMS + ("pool5",)})             # the region head on the GOLDEN's rois
    assert p["pool5"].shape == (n, 512, 7, 7) and p["fc7"].shape == (n, 4096)
    p["fc7"] = p["fc7"][:FC7_ROWS]
    for name in TRUNK_SEAMS + HEAD_SEAMS:
        gold = G[f"{case}_{name}"]
        assert p[name].shape == gold.shape and p[name].dtype == np.float32, name
        err, tol = float(np.abs(p[name] - gold).max()), _tolerance(dtype, name, gold)
        print(f"{DTYPE_IDS[DTYPES.index(dtype)]} case {case} {name}: max abs {err:.3e}, tolerance {tol:.3e} ({err / tol:.3f} of it)")
        assert err <= tol, (name, err, tol)
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
    # extract_head: net_conv alone
    head = net.extract_head(plan.x_static.cpu().numpy().transpose(0, 2, 3, 1))
    assert tuple(head.shape) == (1, 512, fh, fw) and head.dtype == torch.float32


@pytest.mark.parametrize("case", CASES)
def test_fc_and_igemm_heads_agree(hip_lib, case):
    """fp16: classifier.0 / .3 pinned to ft_fc_fwd and to ft_conv2d_fwd, on the golden's RoIs.  Each form's fc7 lies inside the
    derived bound of two fp16 layers (detect_vgg_ref.two_layer_bound) around the float64 result of ITS OWN pool5 and the fp16
    weights; so the two differ by at most the two bounds plus what their float64 results differ by (zero when the two trunks
    produced the same pool5 bits)."""
    sd = _state_dict()
    w1 = sd["vgg.classifier.0.weight"].view(4096, 512, 7, 7).permute(0, 2, 3, 1).reshape(4096, -1).half()          # (h, w, c), as pool5 lies
    w2 = sd["vgg.classifier.3.weight"].half()
    b1, b2 = sd["vgg.classifier.0.bias"], sd["vgg.classifier.3.bias"]
    rois = torch.from_numpy(G[case + "_rois"]).cuda()
    out = {}
    for form in ("fc", "igemm"):
        net = _net(torch.float16, form)
        plan, im_info, shape, _ = _run(net, case, keep=False)
        head = net.region_head(plan, rois, float(im_info[2]), shape, keep_intermediates=True)
        names = [c[0] for c in next(iter(plan.heads.values())).prog.calls]
        assert (names.count("ft_fc_fwd") == 2) == (form == "fc") and not any(n.startswith("__") for n in names), names
        pool5 = head["pool5"].permute(0, 2, 3, 1).reshape(len(rois), -1).half().cpu()                             # exact: the buffer is fp16
        bound, want = V.two_layer_bound(pool5, w1, b1, w2, b2)
        got = head["fc7"].double().cpu()
        ratio = float(((got - want).abs() / bound).max())
        print(f"case {case} {form}: fc7 max abs {float((got - want).abs().max()):.3e} on values of {float(want.max()):.2f}, {ratio:.3f} of the two-layer bound")
        assert ratio <= 1.0, form
        out[form] = (got, want, bound)
    (ga, wa, ba), (gb, wb, bb) = out["fc"], out["igemm"]
    diff, allowed = (ga - gb).abs(), ba + bb + (wa - wb).abs()
    print(f"case {case}: fc vs igemm fc7 max abs {float(diff.max()):.3e}, {float((diff / allowed).max()):.3f} of the allowance")
    assert bool((diff <= allowed).all())


def test_plan_structure_and_reuse(hip_lib):
    """The trunk's launch list; the fp16 head's classifier layers resolved to ONE form each; a second frame of the same blob shape
    replays both plans, and the same frame again gives the same bits."""
    net = _net(torch.float16)
    plan_a, _, _, a1 = _run(net, "a", keep=False)
    names = [c[0] for c in plan_a.prog.calls]
    assert names[0] == "ft_pack_nchw_to_nhwc" and names.count("ft_maxpool2x2s2_fwd") == 4 and names.count("ft_rpn_softmax_fwd") == 1
    assert sum(n.startswith(("ft_conv2d_fwd", "ft_conv_direct_fwd")) for n in names) == 13 + 2 and not any(n.startswith("__") for n in names)
    assert (plan_a.net_conv.H, plan_a.net_conv.W, plan_a.net_conv.C) == (4, 6, 512)
    head = next(iter(plan_a.heads.values()))
    hnames = [c[0] for c in head.prog.calls]
    assert hnames[0] == "ft_roi_crop_nhwc_fwd" and head.rois.shape == (300, 5) and head.prog.calls[0][1][10] == 1          # max_pool = 1
    assert len(hnames) == 4 and hnames.count("ft_fc_fwd") in (0, 1, 2) and not any(n.startswith("__") for n in hnames), hnames
    runs, hruns, nplans = plan_a.runs, head.runs, len(net._plans)
    assert plan_a.prog.graph_exec is not None and head.prog.graph_exec is not None
    other = np.ascontiguousarray(_frame("a")[::-1, ::-1])                         # another image of the same blob shape
    plan_o, im_info, _, shape = det_test.stage_frame(net, other, TARGET, MAX_SIZE)
    o = net.detect_staged(plan_o, im_info, frame_shape=shape)
    assert plan_o is plan_a and len(net._plans) == nplans and plan_a.runs == runs + 1 and len(plan_a.heads) == 1 and head.runs == hruns + 1
    assert not np.array_equal(o["cls_score"].cpu().numpy(), a1["cls_score"])
    _, _, _, a2 = _run(net, "a", keep=False)
    for k in ("rois", "cls_score", "cls_prob", "bbox_pred", "pred_boxes", "rpn_cls_prob"):
        assert np.array_equal(a1[k].view(np.int32), a2[k].view(np.int32)), k
    with pytest.raises(Exception, match="too small"):
        net.trunk_plan(31, 64)                                                    # 31 // 16 = 1: no 2 x 2 map for the crop
    # fp32 records the implicit GEMM alone
    net32 = _net(torch.float32)
    plan32, _, _, _ = _run(net32, "b", keep=False)
    h32 = [c[0] for c in next(iter(plan32.heads.values())).prog.calls]
    assert "ft_fc_fwd" not in h32 and (plan32.net_conv.H, plan32.net_conv.W) == (3, 7)


def test_demo_tool(hip_lib, tmp_path, capsys):
    import sys
    sys.path.insert(0, ROOT)
    from tools.detection import demo
    frame = synth.detector_frame(SEED, 50, 72)
    path = tmp_path / "frame.ppm"
    path.write_bytes(b"P6\n72 50\n255\n" + np.ascontiguousarray(frame[:, :, ::-1]).tobytes())          # PPM is RGB
    dets = demo.main(["--net", "vgg16", "--num_classes", "3", "--person_id", "1", "--image", str(path), "--target_size", "75",
                      "--max_size", "125", "--seed", str(SEED)])
    out = capsys.readouterr().out
    assert dets.ndim == 2 and dets.shape[1] == 5 and np.isfinite(dets).all() and f"{len(dets)} person boxes" in out
    want = det_test.detect_persons(_net(torch.float32), frame, PERSON, 0.3, target_size=TARGET, max_size=MAX_SIZE)
    assert np.array_equal(dets, want)
