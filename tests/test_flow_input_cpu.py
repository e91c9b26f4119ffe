"""Self-test of tests/flow_input_ref.py, the inputs and reference of tests/test_flow_input_gpu.py: the integer frames really make
every fp32 summation order exact, one lost or doubled pixel / row / group / split really moves the expected mean, and the
restated work splits give the workgroup counts and row shares the GPU module places its impulses by.  Nothing on the GPU is
judged here."""
import numpy as np
import pytest

import flow_input_ref as R
from flow_input_ref import F32

CASES = R.SHAPES + [R.GRID_CAP_CASE]
IDS = [R.sid(c) for c in CASES]


def _sets(case):
    B, H, W = case
    return [R.int_pairs(rep, B, H, W) for rep in range(R.FUSED_SETS)]


def _tree(v):
    """Pairwise (butterfly-like) float32 reduction of a power-of-two vector."""
    v = np.asarray(v, dtype=F32)
    while v.size > 1:
        v = (v[:v.size // 2] + v[v.size // 2:]).astype(F32)
    return v[0]


def _strided(v, n):
    """n strided lanes, each summed sequentially in float32, then the lanes by a tree."""
    pad = (-v.size) % n
    lanes = np.concatenate([v, np.zeros(pad, F32)]).reshape(-1, n)
    return _tree(np.cumsum(lanes, axis=0, dtype=F32)[-1])


def _float4_lanes(v):
    """rgb_partial_sum_kernel's shape: float4 j goes to lane j % 256, accumulator (j / 256) % 4; per component sequential;
    (a0 + a1) + (a2 + a3); (c0 + c1) + (c2 + c3); the lanes by a tree."""
    pad = (-v.size) % (4 * 256 * 4)
    q = np.concatenate([v, np.zeros(pad, F32)]).reshape(-1, 4, 256, 4)       # [round, accumulator, lane, component]
    a = np.cumsum(q, axis=0, dtype=F32)[-1]
    a = ((a[0] + a[1]).astype(F32) + (a[2] + a[3]).astype(F32)).astype(F32)  # [lane, component]
    s = ((a[:, 0] + a[:, 1]).astype(F32) + (a[:, 2] + a[:, 3]).astype(F32)).astype(F32)
    return _tree(s)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integer_frames_are_exact_in_every_order(case):
    B, H, W = case
    vm = R.vmax(H, W)
    sets = _sets(case)
    sums = [R.colour_sums(x) for x in sets]
    for x, S in zip(sets, sums):
        assert x.dtype == F32 and x.shape == (B, 3, 2, H, W)
        assert np.array_equal(x, np.rint(x)) and x.min() >= 1 and x.max() <= vm
        assert S.max() < R.SUM_LIMIT
        m = R.expected_mean(x)
        assert m.dtype == F32 and len(set(m.tolist())) == 3 * B, "two (sample, colour) means coincide"
    # the frame sets of the fused kernel's test differ in every (sample, colour) sum
    per_slot = np.stack([S.reshape(-1) for S in sums])
    for k in range(3 * B):
        assert len(set(per_slot[:, k].tolist())) == R.FUSED_SETS
    x, S = sets[0], sums[0].reshape(-1)
    rng = np.random.default_rng(3)
    for k in range(3 * B):
        v = x.reshape(3 * B, -1)[k]
        got = (np.cumsum(v, dtype=F32)[-1], _strided(v, 64), _strided(v, 256), _float4_lanes(v),
               np.cumsum(v[rng.permutation(v.size)], dtype=F32)[-1])
        assert all(g.dtype == F32 and int(g) == int(S[k]) and float(g) == float(S[k]) for g in got), (k, got, S[k])
    # the exact partial sums the GPU module expects add up to the same integers
    assert np.array_equal(R.split_sums(x).astype(np.int64).sum(1), S)
    assert np.array_equal(R.chunk_sums(x).astype(np.int64).sum(1), S)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_mutation_moves_the_expected_mean(case):
    B, H, W = case
    x = R.int_pairs(0, B, H, W)
    want = R.expected_mean(x)
    rng = np.random.default_rng(7)
    for i in range(16):
        kind = R.MUTATIONS[i % len(R.MUTATIONS)]
        y, k = R.mutate(x, kind, rng)
        got = R.expected_mean(y)
        assert got[k] != want[k], (kind, k)
        assert np.array_equal(np.delete(got, k), np.delete(want, k))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adjacent_sums_give_different_means(case):
    _, H, W = case
    S = np.arange(0, R.vmax(H, W) * 2 * H * W + 2, dtype=np.int64)
    m = R.mean_of_sums(S, H, W)
    assert m.dtype == F32 and np.all(np.diff(m) > 0)


def test_expected_mean_and_layouts_on_a_hand_case():
    x = np.zeros((1, 3, 2, 1, 4), dtype=F32)
    x[0, 0, 0, 0] = (1, 2, 3, 4)
    x[0, 0, 1, 0] = (5, 6, 7, 8)
    x[0, 1] = 2
    x[0, 2] = 3
    m = R.expected_mean(x)
    assert np.array_equal(m, np.array([4.5, 2.0, 3.0], dtype=F32))
    xn = R.normalise(x, m, 256.0)
    v6, v3 = R.view6(xn, 1, 6, np.float32), R.view3(xn, 1, 6, np.float16)
    assert v6.shape == (1, 1, 6, 8) and v3.shape == (2, 1, 6, 4)
    assert np.array_equal(v6[0, 0, 1], np.array([-3.5 / 256, 0, 0, 0.5 / 256, 0, 0, 0, 0], dtype=F32))
    assert not v6[0, 0, 0].any() and not v6[0, 0, 5].any() and not v3[:, 0, (0, 5)].any()
    assert np.array_equal(v3[1, 0, 4], np.array([3.5 / 256, 0, 0, 0], dtype=np.float16))
    fv = R.fold_view(x, m, 1, 7, 256.0)
    assert fv.shape == (1, 3, 7, 8)
    assert np.array_equal(fv[0, 1, 2], np.array([2 / 256, 2 / 256, 3 / 256, 6 / 256, 2 / 256, 3 / 256, 0, 0], dtype=np.float16))
    pad = np.array([4.5 / 256, 2 / 256, 3 / 256, 4.5 / 256, 2 / 256, 3 / 256, 0, 0], dtype=np.float16)
    for (r, c) in ((0, 0), (0, 3), (2, 6), (1, 0), (1, 5), (1, 6)):
        assert np.array_equal(fv[0, r, c], pad)
    sh = R.fold_shift(m, np.ones((2, 8)), None, np.array([1.0, 2.0]), 256.0)
    assert np.allclose(sh, np.array([[1.0, 2.0]]) - 2 * (4.5 + 2 + 3) / 256, atol=1e-12)


def test_impulse_frames():
    x = R.impulse_pairs(1, 3, 4, [(0, 0, 0), (1, 2, 3), (0, 1, 2)])
    assert x.sum() == 3 * R.vmax(3, 4) and x[0, 0, 0, 0, 0] == x[0, 1, 1, 2, 3] == x[0, 2, 0, 1, 2] == R.vmax(3, 4)
    for pos in (R.mean_impulse_positions, R.fold_impulse_positions):
        for (_, H, W) in R.SHAPES:
            for launch in R.impulse_launches(H, W, pos(H, W)):
                assert len(launch) % 3 == 0 and 3 <= len(launch) <= 48
                assert len(launch) // 3 * 24 * H * W <= 13 * 2 ** 20


def test_impulse_views_match_the_general_path():
    for (H, W) in ((3, 4), (13, 512), (7, 2048)):
        for launch in R.impulse_launches(H, W, R.fused_impulse_positions(H, W)):
            B = len(launch) // 3
            x = R.impulse_pairs(B, H, W, launch)
            assert np.array_equal(R.expected_mean(x), R.impulse_mean(B, H, W))
            xn = R.normalise(x, R.expected_mean(x))
            for dtype in (np.float16, np.float32):
                v6, v3 = R.impulse_views(B, H, W, launch, 3, W + 6, 1, W + 5, dtype)
                assert np.array_equal(v6, R.view6(xn, 3, W + 6, dtype)) and np.array_equal(v3, R.view3(xn, 1, W + 5, dtype))


def test_fp16_subnormals_are_among_the_expected_values():
    """Where the mean lies within 0.0156 of a pixel value, (x - mean) / 255 is an fp16 subnormal: the GPU module's bit-equal views
    hold hundreds of thousands of them (numpy rounds them to nearest even), so a kernel that flushed them would fail there."""
    for (B, H, W), least in (((2, 13, 512), 100), ((2, 5, 6144), 1000), ((3, 160, 832), 100000), ((2, 42, 6144), 100000)):
        x = R.int_pairs(0, B, H, W)
        h = R.normalise(x, R.expected_mean(x)).astype(np.float16)
        assert int(((np.abs(h) < np.float16(2.0 ** -14)) & (h != 0)).sum()) >= least, (B, H, W)


@pytest.mark.parametrize("case", R.SHAPES, ids=[R.sid(c) for c in R.SHAPES])
def test_impulse_positions_cover_the_named_ones(case):
    _, H, W = case
    HW, L = H * W, 2 * H * W
    pos = set(R.mean_impulse_positions(H, W))
    assert {(0, 0, 0), (0, H - 1, W - 1), (1, 0, 0), (1, H - 1, W - 1)} <= pos
    per = -(-L // 64)
    for s in (0, 1, 31, 63):
        lo, hi = s * per, min(L, (s + 1) * per)
        if lo < L:
            for p in (lo, hi - 1):
                assert (p // HW, p % HW // W, p % W) in pos, (s, p)
    if (H, W) == (160, 832):
        # 1040 float4 per split: lanes 0..255 take float4 0..1023 in the unrolled loop, lanes 0..15 float4 1024..1039 in the tail
        assert per == 4160 and {(0, 4095 // W, 4095 % W), (0, 4096 // W, 4096 % W)} <= pos
    if W % 4 == 0:
        fpos = set((y, x) for _, y, x in R.fold_impulse_positions(H, W))
        n = (H + 3) // 4
        for ch in (0, n // 2, n - 1):
            assert {(4 * ch, 0), (min(H, 4 * ch + 4) - 1, W - 1)} <= fpos
        upos = set((y, x) for _, y, x in R.fused_impulse_positions(H, W))
        r0 = 0
        for rows in R.fused_row_shares(H, W):
            assert {(r0, 0), (r0 + rows - 1, W - 1)} <= upos
            r0 += rows
        assert r0 == H


def test_work_splits_restated():
    shares = {
        (1, 4): [1], (3, 4): [3], (5, 26): None, (7, 9): None, (9, 40): [9], (11, 8): [11],
        (13, 512): [7, 6], (25, 512): [9, 9, 7], (7, 2048): [3, 3, 1], (5, 6144): [1] * 5,
        (130, 100): [44, 44, 42], (50, 260): [17, 17, 16], (160, 832): [7] * 22 + [6], (42, 6144): [1] * 42,
    }
    assert set(shares) == {(H, W) for _, H, W in R.SHAPES}
    for (H, W), want in shares.items():
        if want is None:
            assert R.fused_plan(H, W) is None
        else:
            assert R.fused_row_shares(H, W) == want and sum(want) == H
            assert max(want) * (W // 4) <= R.FUSED_ITEMS            # a workgroup's share fits its registers
    assert R.fused_row_shares(5, 6144) == [1] * 5 and 6144 // 4 == R.FUSED_ITEMS
    # refusals: more than 42 workgroups (3 n > 128), W % 4 != 0, W < 4; the grid cap of 512 resident workgroups
    assert R.fused_plan(43, 6144) is None and R.fused_plan(7, 9) is None and R.fused_plan(8, 2) is None
    assert R.fused_state_words(2, 42, 6144) == 2 * 4 * 42 + 1 and R.fused_state_words(2, 43, 6144) == 0
    assert R.fused_state_words(512, 1, 4) == 512 * 4 + 1 and R.fused_state_words(513, 1, 4) == 0
    assert R.fused_state_words(12, 42, 6144) == 12 * 4 * 42 + 1 and R.fused_state_words(13, 42, 6144) == 0
    # which mean path a shape takes, and how many splits are empty
    vec = {(H, W): R.mean_path_is_vector(H, W) for _, H, W in R.SHAPES}
    assert vec[(9, 40)] and not vec[(11, 8)] and not vec[(5, 26)] and not vec[(7, 9)] and vec[(160, 832)] and vec[(42, 6144)]
    assert not vec[(1, 4)] and not vec[(3, 4)]
    empty = {(H, W): sum(hi <= lo for lo, hi in R.split_spans(H, W)[1]) for _, H, W in R.SHAPES}
    assert empty[(1, 4)] == 56 and empty[(3, 4)] == 40 and empty[(9, 40)] == 4 and empty[(11, 8)] == 5
    # 42 x 6144: 2016 float4 per split = one full unrolled round (1024) + one that lanes 0..223 take (224 + 768 = 992 < 2016 - 1024)
    per, _ = R.split_spans(42, 6144)
    assert per == 8064 and per // 4 == 2016
    # fold chunks: 9 = 4 + 4 + 1, 11 = 4 + 4 + 3
    assert R.fold_chunks(9) == 3 and R.fold_chunks(11) == 3 and R.fold_chunks(1) == 1 and R.fold_chunks(160) == 40
    # the grid-cap batch is the scalar pack kernel's: one thread per view pixel
    B, H, W = R.GRID_CAP_CASE
    assert W % 4 and R.GRID_CAP_THREADS < B * H * (W + 1) <= R.GRID_CAP_THREADS + 4096
