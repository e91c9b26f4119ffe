"""The references and case tables of tests/keypoint_ref.py pinned on the CPU before they judge the HIP kernels
(tests/test_keypoint_gpu.py): against the oracle's restatement of max_preds / final_preds, against torch on the CPU, against the
flag set and statistics test_argmax_screen_is_selective states for its own input, and — a condition on the cases, not a
measurement — every decision of every screen case sits at least 1.5x away from its threshold."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import keypoint_ref as R
from conftest import GOLDEN
from oracle import keypoints_ref

SIZES = pytest.mark.parametrize("size", R.MAX_PREDS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")


def _oracle(hm, adjust):
    N = hm.shape[0]
    _, scores, idx, pre = keypoints_ref.final_preds_ref(hm, np.zeros((N, 2)), np.full(N, float(hm.shape[2])), adjust_coords=bool(adjust))
    return idx, scores[..., 0], pre


def _assert_is_the_oracle(hm, adjust):
    idx, score, coords = R.max_preds_ref64(hm, adjust)
    o_idx, o_score, o_pre = _oracle(hm, adjust)
    assert np.array_equal(idx, o_idx) and np.array_equal(score.view(np.int32), o_score.view(np.int32))
    assert coords.dtype == np.float32 and np.array_equal(coords, o_pre.astype(np.float32))


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("layout", R.MAX_PREDS_LAYOUTS)
@SIZES
def test_max_preds_ref_is_the_oracle_on_every_case(size, layout, adjust):
    hm, _ = R.max_preds_case(*size, layout)
    _assert_is_the_oracle(hm, adjust)


@pytest.mark.parametrize("adjust", [0, 1])
def test_max_preds_ref_is_the_oracle_on_the_golden_heatmaps(adjust):
    hm = np.load(os.path.join(GOLDEN, "pose_golden.npz"))["r50_heatmaps_b2"]
    _assert_is_the_oracle(np.ascontiguousarray(hm, dtype=np.float32), adjust)


@SIZES
def test_max_preds_plants_are_what_their_names_say(size):
    """Answers known by construction: a wrong case table must not pass for a thorough one."""
    H, W = size
    HW = H * W
    names, maps = R.max_preds_plants(H, W)
    idx, score, coords = R.max_preds_ref64(maps[:, None], 1)
    got = {n: (int(idx[i, 0]), float(score[i, 0]), tuple(coords[i, 0].tolist())) for i, n in enumerate(names)}
    first = {"tie_same_thread": 5, "tie_lanes": 10, "tie_waves": 100, "tie_first_last": 0, "tie_three": 1, "tie_three_waves": 200,
             "max_last": HW - 1, "all_equal": 0, "all_equal_negative": 0, "max_zero": HW // 2, "max_negative_zero": HW // 2,
             "max_subnormal": HW // 2, "negative_zero_ties_zero": 1}
    for name, want in first.items():
        if name in got:
            assert got[name][0] == want, name
    if HW > 300:
        assert {"tie_same_thread", "tie_lanes", "tie_waves"} <= set(names)
    for name in ("max_zero", "max_negative_zero", "all_equal_negative", "negative_zero_ties_zero"):
        if name in got:
            assert got[name][2] == (0.0, 0.0), name                    # the mask: score > 0 does not hold
    i_sub = names.index("max_subnormal")                                  # > 0 for numpy: the coordinates are kept
    assert score[i_sub, 0] == R.SUBNORMAL > 0
    assert tuple(R.max_preds_ref64(maps[i_sub][None, None], 0)[2][0, 0].tolist()) == (float((HW // 2) % W), float((HW // 2) // W))
    assert np.signbit(maps[names.index("max_negative_zero")].reshape(-1)[HW // 2])
    if "negative_zero_ties_zero" in got:
        assert np.signbit(score[names.index("negative_zero_ties_zero"), 0])
    if H >= 3 and W >= 3:
        yc, xc = H // 2, W // 2
        want = {"nudge_dx0": (xc, yc + 0.25), "nudge_dy0": (xc - 0.25, yc), "nudge_equal_neighbours": (xc, yc),
                "nudge_x1": (0.75, yc + 0.25), "nudge_xW2": (W - 2 + 0.25, yc - 0.25), "nudge_y1": (xc - 0.25, 0.75),
                "nudge_yH2": (xc + 0.25, H - 2 + 0.25)}
        for name, c in want.items():
            assert got[name][2] == c, name
    for name in names:
        if name.startswith("border_"):
            x, y = got[name][2]
            assert x == int(x) and y == int(y) and (x in (0, W - 1) or y in (0, H - 1)), name
    # the batch-index check of the GPU test needs crops whose answers differ
    for layout in R.MAX_PREDS_LAYOUTS:
        hm, _ = R.max_preds_case(H, W, layout)
        i2, s2, c2 = R.max_preds_ref64(hm, 1)
        assert hm.shape[0] >= 2 and not (np.array_equal(i2[0], i2[1]) and np.array_equal(s2[0], s2[1]))


def test_top2_ref_is_topk():
    for shape in R.SCREEN_SHAPES:
        hm, _ = R.screen_case(*shape)
        _, _, finite, _ = R.screen_ref(hm, R.SCREEN_REL)
        t1, t2 = R.top2_ref(hm[finite])
        want = torch.from_numpy(hm[finite]).flatten(2).topk(2, dim=2).values.double().numpy()
        assert np.array_equal(t1, want[..., 0]) and np.array_equal(t2, want[..., 1])
    tie = np.array([[[[1.0, 3.0], [3.0, 2.0]]]], dtype=np.float32)
    assert R.top2_ref(tie)[0][0, 0] == 3.0 and R.top2_ref(tie)[1][0, 0] == 3.0


def test_screen_ref_reproduces_the_selective_test():
    """The flag set and the statistics tests/test_pose_gpu.py::test_argmax_screen_is_selective asserts of the kernel, asserted of
    the reference on the same input."""
    hm, rel, special = R.selective_screen_input()
    flags, st, finite, _ = R.screen_ref(hm, rel)
    assert sorted(np.flatnonzero(flags).tolist()) == sorted(special)
    assert sorted(np.flatnonzero(~finite).tolist()) == [11, 13]
    clean = [n for n in range(hm.shape[0]) if n not in special]
    t = torch.from_numpy(hm[clean])
    top2 = t.flatten(2).topk(2, dim=2).values
    assert np.array_equal(st[clean, 0], (top2[..., 0] - top2[..., 1]).min(dim=1).values.numpy())
    rng = (t.flatten(1).max(dim=1).values - t.flatten(1).min(dim=1).values).numpy()
    assert np.array_equal(st[clean, 1], rng) and np.allclose(st[clean, 3], rel * rng, rtol=0, atol=1e-7)
    assert np.array_equal(st[clean, 3], np.float32(rel) * rng)
    assert np.array_equal(st[clean, 2], top2[..., 0].abs().min(dim=1).values.numpy())
    assert (st[clean, 0] > 20 * st[clean, 3]).all()
    assert st[3, 0] < 2 * st[3, 3] and st[7, 2] < st[7, 3]                  # why crops 3 and 7 are flagged


@pytest.mark.parametrize("shape", R.SCREEN_SHAPES, ids=str)
def test_screen_cases_keep_their_distance_from_the_thresholds(shape):
    """CONDITION ON THE CASES: for every finite crop of every screen case, the margin of every map is at least 1.5x above 2 E or
    at least 1.5x below it, and |top-1| likewise against E — so no decision of the GPU test hangs on a last bit — and each kind
    of crop lands on the side it was planted on."""
    K, H, W, offset = shape
    hm, kinds = R.screen_case(*shape)
    assert hm.shape[0] == len(kinds) >= 3
    flags, stats, finite, dist = R.screen_ref(hm, R.SCREEN_REL)
    assert [k for k, f in zip(kinds, finite) if not f] == [k for k in kinds if k.split("_")[0] in ("nan", "posinf", "neginf")]
    for name in ("margin_over_2E", "abs_over_E"):
        d = dist[name][finite]
        assert d.shape == (int(finite.sum()), K) and not np.isnan(d).any()
        assert ((d >= 1.5) | (d <= 1.0 / 1.5)).all(), (name, d[(d < 1.5) & (d > 1.0 / 1.5)])
    flagged_kinds = {"max_near_zero"} if H * W == 2 else R.SCREEN_FLAGGED_KINDS      # two pixels: margin = R, never inside 2 E
    for n, kind in enumerate(kinds):
        assert bool(flags[n]) == (not finite[n] or kind in flagged_kinds), kind
        if finite[n] and H * W > 2:
            m, a = dist["margin_over_2E"][n], dist["abs_over_E"][n]
            assert (m < 1).sum() == (kind in ("tie", "near_tie")) and (a < 1).sum() == (kind == "max_near_zero"), kind
            assert stats[n, 0] == 0.0 if kind == "tie" else stats[n, 0] > 0.0
            assert 4.0 <= stats[n, 1] <= 4.1                                      # R spans map 0 (smallest) and map K - 1 (largest)
    f0, s0, _, _ = R.screen_ref(hm, 0.0)
    assert np.array_equal(f0 != 0, ~finite), "rel_bound = 0 flags only the non-finite crops"


def test_gather_ref_by_hand():
    src = np.arange(20, dtype=np.int32).reshape(5, 4)
    hdr, rows = R.gather_ref(np.array([0, 7, 0, -1, 1], dtype=np.int32), src)
    assert hdr.tolist() == [3, 1, 3, 4] and hdr.dtype == np.int32 and np.array_equal(rows, src[[1, 3, 4]])
    hdr, rows = R.gather_ref(np.zeros(5, dtype=np.int32), src)
    assert hdr.tolist() == [0] and rows.shape == (0, 4)
    for N in R.GATHER_NS:
        pats = R.gather_patterns(N)
        assert int(pats["all"].sum()) == N and not pats["none"].any() and all(p.shape == (N,) and p.dtype == np.int32 for p in pats.values())
        assert np.flatnonzero(pats["rows_ge_256"]).tolist() == list(range(256, N))
        assert set(np.unique(pats["half_value_7"]).tolist()) <= {0, 7} and set(np.unique(pats["half_value_minus_1"]).tolist()) <= {0, -1}


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_bn_ref_is_torch_batch_norm_in_float64(fp16):
    """F.batch_norm(training=True, momentum=1) leaves the batch mean and the UNBIASED batch variance in the running statistics."""
    cases = [(R.bn_exact_input(s), s) for s in R.BN_EXACT_SHAPES] + [(R.bn_random_input(s, fp16), s) for s in R.BN_RANDOM_SHAPES]
    cases.append((R.bn_impulse_input()[0], R.BN_IMPULSE_SHAPE))
    for buf, (N, H, W, C, cs) in cases:
        x = torch.from_numpy(buf[..., :C])
        x = x.half() if fp16 else x
        mean, var = R.bn_ref64(x)
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        F.batch_norm(x.double().permute(0, 3, 1, 2), rm, rv, training=True, momentum=1.0)
        n = N * H * W
        tol = (n + 8) * 2.0 ** -52                      # two float64 sums of n addends, any order: (n - 1) 2^-53 of the sum of magnitudes each
        assert np.abs(mean - rm.numpy()).max() <= tol * max(1.0, np.abs(x.double().numpy()).mean())
        assert np.abs(var * n / (n - 1) - rv.numpy()).max() <= tol * max(1.0, (x.double().numpy() ** 2).mean())
        assert (buf[..., C:] == R.BN_GUARD).all()
    buf, p = R.bn_impulse_input()
    N, H, W, C, cs = R.BN_IMPULSE_SHAPE
    mean, _ = R.bn_ref64(buf[..., :C])
    assert np.abs(mean - 1.0 / (N * H * W)).max() <= 1e-18 and p[:4].tolist() == [0, 7, 8, N * H * W - 1]
