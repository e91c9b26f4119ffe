"""The CPU side of detection.nets.vgg16: the restatement (tests/detect_vgg_ref.py) against the reference's recorded run
(tests/golden/detect_vgg_golden.npz), the state_dict contract, the refusal codes of the new entry points (no device needed: a
refused call launches nothing) and the properties that make the exact FC cases exact."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import detect_net_ref as R
import detect_vgg_ref as V
from conftest import GOLDEN
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_F16, FT_F32, FT_OK, FlowtrackHipError
from flowtrack.pytorch_amd.detection import nets

G = np.load(os.path.join(GOLDEN, "detect_vgg_golden.npz"), allow_pickle=False)
SEED, TARGET, MAX_SIZE = int(G["seed"]), int(G["target_size"]), int(G["max_size"])
K, PERSON, FC7_ROWS = int(G["num_classes"]), int(G["person_id"]), int(G["fc7_rows"])
CASES = ("a", "b")
CONTINUOUS = ("blob", "net_conv", "rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "rois", "fc7", "cls_score", "cls_prob", "bbox_pred",
              "scores", "pred_boxes")
P, NULL = ctypes.c_void_p(0x1000), None
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)


@functools.lru_cache(maxsize=None)
def _net():
    net = nets.vgg16()
    net.create_architecture(K, tag="default")
    return net


@functools.lru_cache(maxsize=None)
def _state_dict():
    return synth.fill_vgg_detector_state_dict(_net().state_dict(), SEED)


def _frame(case):
    h, w = (int(v) for v in G[case + "_frame_hw"])
    return synth.detector_frame(SEED, h, w)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    mine = V.im_detect(_state_dict(), _frame(case), TARGET, MAX_SIZE)
    mine["fc7"] = mine["fc7"][:FC7_ROWS]
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
    """The conditions the golden's seed was searched for, on the stored tensors; the map sizes the pools meet."""
    A = G[case + "_rpn_cls_prob"].shape[-1] // 2
    fg, pp = G[case + "_rpn_cls_prob"][..., A:], G[case + "_cls_prob"][:, PERSON]
    assert np.abs(G[case + "_net_conv"]).max() <= 32 and np.abs(G[case + "_fc7"]).max() <= 32
    assert ((fg > 0.1) & (fg < 0.9)).mean() >= 0.25 and ((pp > 0.1) & (pp < 0.9)).mean() >= 0.25
    assert np.unique(fg).size == fg.size
    assert np.abs(G[case + "_rpn_bbox_pred"]).max() <= 1 and np.abs(G[case + "_bbox_pred"]).max() <= 1
    assert 8 <= len(G[case + "_rois"]) < fg.size
    assert 2 <= len(G[case + "_persons"]) < len(G[case + "_rois"])
    assert G[case + "_fc7"].shape == (FC7_ROWS, 4096) and (G[case + "_fc7"] > 0).any()
    hb, wb = G[case + "_blob"].shape[2:]
    assert G[case + "_net_conv"].shape == (1, 512, V.map_sizes(hb)[3], V.map_sizes(wb)[3])
    assert (hb, wb) == ((75, 108) if case == "a" else (52, 125))
    assert V.map_sizes(75) == (37, 18, 9, 4) and V.map_sizes(108) == (54, 27, 13, 6)        # odd maps 37, 27, 9 and 13 meet a pool
    assert V.map_sizes(52) == (26, 13, 6, 3) and V.map_sizes(125) == (62, 31, 15, 7)        # and 125, 13, 31 and 15


def test_state_dict_keys_and_shapes():
    sd = _net().state_dict()
    keys, shapes = [str(k) for k in G["keys"]], [str(s) for s in G["shapes"]]
    assert list(sd) == keys
    assert [";".join(str(d) for d in sd[k].shape) for k in keys] == shapes
    want = [f"vgg.features.{i}.{p}" for i in CONV_IDX for p in ("weight", "bias")] + [f"vgg.classifier.{i}.{p}" for i in (0, 3) for p in ("weight", "bias")] + \
        [f"{h}.{p}" for h in ("rpn_net", "rpn_cls_score_net", "rpn_bbox_pred_net", "cls_score_net", "bbox_pred_net") for p in ("weight", "bias")]
    assert keys == want and not any(k.startswith("vgg.classifier.6") for k in keys)
    assert tuple(sd["vgg.classifier.0.weight"].shape) == (4096, 25088) and tuple(sd["cls_score_net.weight"].shape) == (K, 4096)
    net = _net()
    assert net._net_conv_channels == 512 and net._fc7_channels == 4096 and net._feat_stride == [16]


def test_load_state_dict_rule_and_pretrained_cnn():
    net = nets.vgg16()
    net.create_architecture(K, tag="default")
    small = {k: v for k, v in _state_dict().items() if k != "vgg.classifier.0.weight"}       # (the 411 MB matrix is not copied about)
    sd = dict(small)
    sd["vgg.classifier.0.weight"] = net.state_dict()["vgg.classifier.0.weight"]
    sd["vgg.classifier.6.weight"], sd["vgg.classifier.6.bias"] = torch.zeros(1000, 4096), torch.zeros(1000)      # an extra key is ignored
    net.load_state_dict(sd)
    got = net.state_dict()
    assert all(torch.equal(got[k], small[k]) for k in small)
    del sd["rpn_net.bias"]
    with pytest.raises(KeyError):
        net.load_state_dict(sd)
    # an ImageNet dict: the keys of `vgg` without the prefix, classifier.6 included, a missing key left alone
    trunk = nets.vgg16()
    trunk.create_architecture(K, tag="default")
    before = trunk.state_dict()["vgg.features.28.bias"].clone()
    imagenet = {k[len("vgg."):]: v for k, v in small.items() if k.startswith("vgg.") and k != "vgg.features.28.bias"}
    imagenet["classifier.6.weight"], imagenet["classifier.6.bias"] = torch.zeros(1000, 4096), torch.zeros(1000)
    trunk.load_pretrained_cnn(imagenet)
    after = trunk.state_dict()
    assert torch.equal(after["vgg.features.0.weight"], small["vgg.features.0.weight"])
    assert torch.equal(after["vgg.classifier.3.weight"], small["vgg.classifier.3.weight"])
    assert torch.equal(after["vgg.features.28.bias"], before) and "vgg.classifier.6.weight" not in after


def test_unsupported_requests():
    net = _net()
    blob = np.zeros((1, 32, 32, 3), dtype=np.float32)
    with pytest.raises(FlowtrackHipError, match="vgg16"):
        net.forward(blob, np.array([32, 32, 1], dtype=np.float32), None, mode="TRAIN")
    with pytest.raises(FlowtrackHipError):
        net.forward(blob, np.array([32, 32, 1], dtype=np.float32), np.zeros((1, 5), dtype=np.float32), mode="TEST")
    with pytest.raises(FlowtrackHipError, match="vgg16"):
        net.train_step({}, None)
    with pytest.raises(FlowtrackHipError, match="create_architecture"):
        nets.vgg16().trunk_plan(64, 64)


def test_synthetic_weights():
    sd = _state_dict()
    again = synth.fill_vgg_detector_state_dict({k: v for k, v in _net().state_dict().items() if k != "vgg.classifier.0.weight"}, SEED)
    assert all(torch.equal(again[k], sd[k]) for k in again)
    w = sd["vgg.classifier.0.weight"]
    a = float(np.sqrt(3.0 * synth.VGG_FC_GAIN / 25088))
    assert float(w.abs().max()) <= a and abs(float(w[:64].std()) / (a / np.sqrt(3.0)) - 1) < 0.01          # U(-a, a): the wanted variance
    w0 = sd["vgg.features.0.weight"]
    assert abs(float(w0.std()) / np.sqrt(synth.VGG_FIRST_CONV_GAIN / 27) - 1) < 0.1
    assert torch.equal(sd["rpn_net.weight"], synth.fill_detector_state_dict({"rpn_net.weight": sd["rpn_net.weight"]}, SEED)["rpn_net.weight"])


# ---- refusal codes --------------------------------------------------------------------------------------------------------------
def test_maxpool2x2_refusals(hip_lib):
    f = lambda x, y, N, H, W, C, dt: hip_lib.ft_maxpool2x2s2_fwd(x, y, N, H, W, C, dt, None)
    for args in ((NULL, P, 1, 4, 4, 8, FT_F16), (P, NULL, 1, 4, 4, 8, FT_F16), (P, P, 0, 4, 4, 8, FT_F16), (P, P, 1, 1, 4, 8, FT_F16),
                 (P, P, 1, 4, 1, 8, FT_F16), (P, P, 1, 4, 4, 0, FT_F16), (P, P, 1, 4, 4, 12, FT_F16), (P, P, 1, 4, 4, 4, FT_F32),
                 (P, P, 1, 4, 4, 8, 7), (ctypes.c_void_p(0x1008), P, 1, 4, 4, 8, FT_F16), (P, ctypes.c_void_p(0x1004), 1, 4, 4, 8, FT_F32),
                 (P, P, -1, 4, 4, 8, FT_F16), (P, P, 1, -4, 4, 8, FT_F16)):
        assert f(*args) == FT_ERR_INVALID_ARG, args
    assert f(P, P, 2, 1024, 1024, 1024, FT_F16) == FT_ERR_UNSUPPORTED                            # 2^31 elements
    assert f(P, P, 1, 32768, 32768, 8, FT_F32) == FT_ERR_UNSUPPORTED


def test_fc_refusals(hip_lib):
    sup, ws, pack = hip_lib.ft_fc_supported, hip_lib.ft_fc_workspace_bytes, hip_lib.ft_fc_pack
    f = lambda dt, x, xs, w, b, y, ys, Rn, k, n, act, wsp, wsb: hip_lib.ft_fc_fwd(dt, x, xs, w, b, y, ys, Rn, k, n, act, wsp, wsb, None)
    assert sup(FT_F16, 300, 25088, 4096, 25088, 4096) == FT_OK and sup(FT_F16, 304, 4096, 4096, 4096, 4096) == FT_OK
    assert sup(FT_F16, 1, 64, 64, 64, 64) == FT_OK and sup(FT_F16, 0, 64, 64, 72, 64) == FT_OK
    assert f(FT_F16, NULL, 64, NULL, NULL, NULL, 64, 0, 64, 64, 1, NULL, 0) == FT_OK                              # zero rows: no launch
    big = 1 << 30
    invalid = ((9, P, 64, P, P, P, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, P, P, P, 64, -3, 64, 64, 0, P, big),
               (FT_F16, P, 64, P, P, P, 64, 3, 0, 64, 0, P, big), (FT_F16, P, 64, P, P, P, 64, 3, 64, -64, 0, P, big),
               (FT_F16, P, 56, P, P, P, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, P, P, P, 56, 3, 64, 64, 0, P, big),
               (FT_F16, P, 68, P, P, P, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, P, P, P, 68, 3, 64, 64, 0, P, big),
               (FT_F16, NULL, 64, P, P, P, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, NULL, P, P, 64, 3, 64, 64, 0, P, big),
               (FT_F16, P, 64, P, P, NULL, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, P, P, P, 64, 3, 64, 64, 0, NULL, big),
               (FT_F16, ctypes.c_void_p(0x1002), 64, P, P, P, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, ctypes.c_void_p(0x1008), P, P, 64, 3, 64, 64, 0, P, big),
               (FT_F16, P, 64, P, ctypes.c_void_p(0x1004), P, 64, 3, 64, 64, 0, P, big), (FT_F16, P, 64, P, P, ctypes.c_void_p(0x1008), 64, 3, 64, 64, 0, P, big),
               (FT_F16, P, 64, P, P, P, 64, 3, 64, 64, 0, ctypes.c_void_p(0x1004), big), (FT_F16, P, 64, P, P, P, 64, 3, 64, 64, 2, P, big),
               (FT_F16, P, 64, P, P, P, 64, 3, 64, 64, -1, P, big), (FT_F16, P, 64, P, P, P, 64, 3, 64, 64, 0, P, ws(3, 64, 64) - 1))
    for args in invalid:
        assert f(*args) == FT_ERR_INVALID_ARG, args
    unsupported = ((FT_F32, 3, 64, 64, 64, 64), (FT_F16, 3, 96, 64, 96, 64), (FT_F16, 3, 64, 96, 64, 96), (FT_F16, 3, 64, 32, 64, 32),
                   (FT_F16, 3, 65536, 32768, 65536, 32768), (FT_F16, 4096, 64, 64, 1 << 20, 64), (FT_F16, 4096, 64, 64, 64, 1 << 20),
                   (FT_F16, 1 << 20, 64, 64, 64, 64))
    for dt, Rn, k, n, xs, ys in unsupported:
        assert sup(dt, Rn, k, n, xs, ys) == FT_ERR_UNSUPPORTED, (dt, Rn, k, n, xs, ys)
        assert f(dt, P, xs, P, P, P, ys, Rn, k, n, 0, P, big) == FT_ERR_UNSUPPORTED
    assert sup(FT_F16, 3, 64, 64, 60, 64) == FT_ERR_INVALID_ARG and sup(5, 3, 64, 64, 64, 64) == FT_ERR_INVALID_ARG
    assert ws(300, 25088, 4096) == 4 * 8 * 300 * 4096 and ws(300, 4096, 4096) == 4 * 8 * 300 * 4096        # 32 column tiles x 8 K-slices = 256 workgroups
    assert ws(0, 64, 64) == 0 and ws(3, 96, 64) == 0 and ws(3, 64, 64) == 4 * 3 * 64
    for args in ((NULL, 64, 64, P), (P, 64, 64, NULL), (ctypes.c_void_p(0x1008), 64, 64, P), (P, 64, 64, ctypes.c_void_p(0x1002)), (P, 0, 64, P), (P, 64, -64, P)):
        assert pack(*args, None) == FT_ERR_INVALID_ARG, args
    for args in ((P, 96, 64, P), (P, 64, 96, P), (P, 32768, 65536, P)):
        assert pack(*args, None) == FT_ERR_UNSUPPORTED, args


# ---- the exact FC cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.FC_EXACT_CASES, ids=lambda c: "R%d_K%d_N%d" % c)
def test_fc_exact_cases_are_exact_and_sensitive(case):
    """Every reference pre-activation and output is an integer of magnitude <= 2048 (exact in fp16; the partial sums, far below
    2^24, exact in fp32 in any order), both signs occur (the ReLU matters), and dropping ONE product changes the result: in the
    first and the last K-step and in the last row and column, so a kernel that loses a K-step, a slice or a tile edge cannot pass."""
    Rn, Kn, Nn = case
    x, w, bias = V.fc_exact_case(*case)
    assert x[:, 0].all() and x[:, -1].all() and w[:, 0].all() and w[:, -1].all()
    assert set(np.unique(x)) <= {-2, -1, 0, 1, 2} and set(np.unique(w)) <= {-1, 0, 1} and np.abs(bias).max() <= 8
    pre = V.fc_exact_ref(*case)
    assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() <= V.FC_EXACT_MAX
    assert np.array_equal(V.fc_ref(x, w, bias, relu=True)[0], np.maximum(pre, 0))
    if pre.size >= 64:
        assert (pre > 0).any() and (pre < 0).any()
    prod = x[:, None, :].astype(np.int32)[-1:] * w[None, -1:, :].astype(np.int32)            # the last row x the last column: [1,1,K]
    for lo, hi in ((0, 64), (Kn - 64, Kn)):
        ks = np.nonzero(prod[0, 0, lo:hi])[0]
        assert len(ks), f"no live product in K-step [{lo}, {hi}) of the last row / column"
        k = lo + int(ks[0])
        x2 = x.copy()
        x2[-1, k] = 0
        assert V.fc_ref(x2[-1:], w[-1:], bias[-1:])[1][0, 0] != pre[-1, -1]
