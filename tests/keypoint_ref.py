"""High-precision CPU references and seeded case tables for the pose-side helper kernels: heat maps -> key points
(ft_heatmap_max_preds / ft_heatmap_keypoint_rows), the arg-max screen of the exact mode (ft_heatmap_argmax_screen,
ft_heatmap_min_margin), the device-side compaction of its re-run set (ft_gather_flagged_rows), the BatchNorm batch statistics
(ft_bn_batch_stats) and the batched person crop (ft_crop_affine_fwd).  TEST INFRASTRUCTURE ONLY: plain numpy, float64 wherever
arithmetic happens, no GPU.  tests/test_keypoint_cpu.py pins every reference here (to oracle/keypoints_ref.py, torch on the CPU
and answers known by construction) before tests/test_keypoint_gpu.py judges the kernels with them.

Every case is a pure function of fixed seeds (flowtrack.pytorch_amd.synth), so both test modules see the same bytes."""
import functools

import numpy as np
import torch

from flowtrack.pytorch_amd import synth


# ---- references -------------------------------------------------------------------------------------------------------------
def max_preds_ref64(hm, adjust):
    """max_preds (+ the adjust_coords nudge of final_preds) of FINITE heat maps hm [N,K,H,W] float32, as
    oracle/keypoints_ref.py states them: the first occurrence of the largest value in row-major order, x = idx % W,
    y = idx // W, the coordinates zeroed where score > 0 does not hold, and for an unmasked peak strictly inside the map
    +-0.25 along each axis by the sign of (next - previous) neighbour, 0 where they are equal.  Comparisons and differences in
    float64 (exact for float32 inputs).  -> idx int32 [N,K], score float32 [N,K], coords float32 [N,K,2]."""
    hm = np.asarray(hm)
    assert hm.dtype == np.float32 and hm.ndim == 4 and np.isfinite(hm).all()
    N, K, H, W = hm.shape
    idx = np.zeros((N, K), dtype=np.int32)
    score = np.zeros((N, K), dtype=np.float32)
    coords = np.zeros((N, K, 2), dtype=np.float32)
    for n in range(N):
        for k in range(K):
            m = hm[n, k].astype(np.float64)
            flat = m.ravel()
            i = int(np.flatnonzero(flat == flat.max())[0])
            idx[n, k], score[n, k] = i, hm[n, k].ravel()[i]
            if not flat[i] > 0.0:
                continue
            x, y = i % W, i // W
            cx, cy = float(x), float(y)
            if adjust and 0 < x < W - 1 and 0 < y < H - 1:
                dx, dy = m[y, x + 1] - m[y, x - 1], m[y + 1, x] - m[y - 1, x]
                cx += 0.25 * (int(dx > 0) - int(dx < 0))
                cy += 0.25 * (int(dy > 0) - int(dy < 0))
            coords[n, k] = (cx, cy)
    return idx, score, coords


def top2_ref(hm):
    """Per map of finite hm [N,K,H,W]: the largest value and the second largest at a DIFFERENT pixel (a tie gives the same value
    twice), by selection — no arithmetic, so the float64 results are exact.  -> (t1, t2) float64 [N,K]."""
    hm = np.asarray(hm)
    N, K = hm.shape[:2]
    flat = hm.reshape(N, K, -1).astype(np.float64)
    assert flat.shape[2] >= 2
    top = np.partition(flat, flat.shape[2] - 2, axis=2)[..., -2:]
    return top[..., 1].copy(), top[..., 0].copy()


def screen_ref(hm, rel_bound):
    """ft_heatmap_argmax_screen as include/flowtrack_hip.h states it.  Per crop: R = largest - smallest value over its K maps,
    E = rel_bound * R, flag when any map has !(top1 - top2 >= 2 E) or !(|top1| >= E), or when the crop holds a non-finite
    value; statistics (smallest margin, R, smallest |top1|, E).  Selections in float64; the statistics are numpy float32
    operations in the header's order — ONE subtraction per margin, one for R, one product for E — each a single IEEE operation
    on float32 inputs, so a kernel has to reproduce them bit for bit.
    -> flags int32 [N], stats float32 [N,4] (NaN rows for crops with a non-finite value: only their flag is defined),
       finite bool [N], dist = {"margin_over_2E", "abs_over_E"}: float64 [N,K], each decision quantity over its threshold
       (>= 1 passes; +inf where the threshold is 0 — R = 0, or rel_bound = 0: margin and |top1| are never negative, so no
       rounding of either side can fail it; NaN for non-finite crops)."""
    hm = np.asarray(hm)
    assert hm.dtype == np.float32 and hm.ndim == 4
    N, K = hm.shape[:2]
    rel = np.float32(rel_bound)
    flags = np.zeros(N, dtype=np.int32)
    stats = np.full((N, 4), np.nan, dtype=np.float32)
    finite = np.isfinite(hm.reshape(N, -1)).all(axis=1)
    dist = {"margin_over_2E": np.full((N, K), np.nan), "abs_over_E": np.full((N, K), np.nan)}

    def over(q, t):
        q, t = q.astype(np.float64), np.full(q.shape, float(t))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(t > 0, q / t, np.inf)
    for n in range(N):
        if not finite[n]:
            flags[n] = 1
            continue
        t1, t2 = top2_ref(hm[n:n + 1])
        t1, t2 = t1[0].astype(np.float32), t2[0].astype(np.float32)          # selections: the cast back is exact
        R = np.float32(hm[n].max()) - np.float32(hm[n].min())
        E = rel * R
        assert R.dtype == np.float32 and E.dtype == np.float32
        margin, at = t1 - t2, np.abs(t1)
        assert margin.dtype == np.float32
        two_e = np.float32(2.0) * E                                               # exact: a power of two
        flags[n] = int((~(margin >= two_e)).any() or (~(at >= E)).any())
        stats[n] = (margin.min(), R, at.min(), E)
        dist["margin_over_2E"][n] = over(margin, two_e)
        dist["abs_over_E"][n] = over(at, E)
    return flags, stats, finite, dist


def gather_ref(flags, src):
    """ft_gather_flagged_rows: header = [count, index of every non-zero flag in ascending order], rows = those rows of src."""
    flags = np.asarray(flags)
    picked = np.flatnonzero(flags != 0)
    return np.concatenate(([len(picked)], picked)).astype(np.int32), np.asarray(src)[picked]


def bn_ref64(x):
    """Per-channel mean and BIASED variance over every leading axis of x [..., C], in float64 of the values AS STORED (an fp16
    tensor is widened, never re-rounded)."""
    x = x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    mean = x.mean(axis=0)
    return mean, ((x - mean) ** 2).mean(axis=0)


# ---- ft_heatmap_max_preds / ft_heatmap_keypoint_rows: case table ------------------------------------------------------------------
MAX_PREDS_SIZES = [(1, 1), (1, 7), (9, 1), (8, 6), (7, 9), (16, 16), (17, 19), (64, 48), (96, 72)]
MAX_PREDS_LAYOUTS = ["K1", "K5", "N2"]      # every planted map of a size in one launch: as N x 1, as N x 5 and as 2 x K
PEAK = np.float32(2.0)
SUBNORMAL = np.float32(2.0 ** -149)         # the smallest positive float32: numpy (and evaluation.py) call it > 0


@functools.lru_cache(maxsize=None)
def max_preds_plants(H, W):
    """(names, maps float32 [P,H,W]): one planted map per property, over a background of uniform values in [-1, -0.5).  A plant a
    map is too small for is left out.  The kernel gives element i to thread i % 256 (lane = thread % 64, wave = thread // 64)."""
    HW = H * W
    names, maps = [], []

    def bg(tag):
        return synth.uniform(71, f"mp.{H}x{W}.{tag}", (H, W), -1.0, -0.5).numpy().copy()

    def add(tag, m):
        names.append(tag)
        maps.append(np.ascontiguousarray(m, dtype=np.float32))

    def tie(tag, where):
        if max(where) < HW and len(set(where)) == len(where):
            m = bg(tag)
            m.reshape(-1)[list(where)] = PEAK
            add(tag, m)
    tie("tie_same_thread", (5, 261))                  # i and i + 256: one thread's strided walk sees both
    tie("tie_lanes", (260, 10))                       # wave 0, lanes 4 and 10: the smaller index sits in the higher lane
    tie("tie_waves", (300, 100))                      # i = 300 in wave 0, i = 100 in wave 1: the smaller index in the higher wave
    tie("tie_first_last", (0, HW - 1))
    tie("tie_three", (1, HW // 2, HW - 2))
    tie("tie_three_waves", (200, 300, 520))           # threads 200 (wave 3), 44 (wave 0), 8 (wave 0): the first one is in wave 3
    tie("max_last", (HW - 1,))
    add("all_equal", np.full((H, W), 0.75))
    add("all_equal_negative", np.full((H, W), -0.5))
    pos = HW // 2
    for tag, v in (("max_zero", 0.0), ("max_negative_zero", -0.0), ("max_subnormal", SUBNORMAL)):
        m = bg(tag)
        m.reshape(-1)[pos] = v
        add(tag, m)
    if HW >= 3:                                       # -0.0 == +0.0: the first one is the arg-max and its bits are the score
        m = bg("zeros_tie")
        m.reshape(-1)[1], m.reshape(-1)[HW - 1] = -0.0, 0.0
        add("negative_zero_ties_zero", m)

    def peak(tag, y, x, left, right, up, down):
        m = bg(tag)
        for yy, xx, v in ((y, x - 1, left), (y, x + 1, right), (y - 1, x, up), (y + 1, x, down)):
            if 0 <= yy < H and 0 <= xx < W:
                m[yy, xx] = v
        m[y, x] = PEAK
        add(tag, m)
    yc, xc = H // 2, W // 2
    if H >= 3 and W >= 3:                             # peaks strictly inside: these get the nudge
        peak("nudge_dx0", yc, xc, 0.5, 0.5, 0.3, 0.6)
        peak("nudge_dy0", yc, xc, 0.6, 0.3, 0.5, 0.5)
        peak("nudge_equal_neighbours", yc, xc, 0.5, 0.5, 0.5, 0.5)
        peak("nudge_x1", yc, 1, 1.0, 0.5, 0.2, 0.4)           # the decisive neighbour is a border pixel
        peak("nudge_xW2", yc, W - 2, 0.5, 1.0, 0.4, 0.2)
        peak("nudge_y1", 1, xc, 0.4, 0.2, 1.0, 0.5)
        peak("nudge_yH2", H - 2, xc, 0.2, 0.4, 0.5, 1.0)
    seen = set()
    for tag, y, x in (("top", 0, xc), ("bottom", H - 1, xc), ("left", yc, 0), ("right", yc, W - 1), ("corner_tl", 0, 0),
                      ("corner_tr", 0, W - 1), ("corner_bl", H - 1, 0), ("corner_br", H - 1, W - 1)):
        if (y, x) not in seen:                        # peaks on the border: never a nudge, whatever their neighbours say
            seen.add((y, x))
            peak("border_" + tag, y, x, 0.2, 0.9, 0.3, 0.8)
    for j in range(2):
        add(f"noise_{j}", synth.normal(72, f"mp.noise.{H}x{W}.{j}", (H, W)).numpy())
    out = np.stack(maps)
    out.setflags(write=False)
    return tuple(names), out


@functools.lru_cache(maxsize=None)
def max_preds_case(H, W, layout):
    """hm float32 [N,K,H,W] holding every planted map of (H, W), filled up with noise maps, and the plant names in map order."""
    names, maps = max_preds_plants(H, W)
    P = len(names)
    N, K = {"K1": (P, 1), "K5": (-(-P // 5), 5), "N2": (2, -(-P // 2))}[layout]
    pad = [synth.normal(73, f"mp.pad.{H}x{W}.{layout}.{j}", (H, W)).numpy() for j in range(N * K - P)]
    hm = np.ascontiguousarray(np.concatenate((maps, np.stack(pad))) if pad else maps).reshape(N, K, H, W)
    hm.setflags(write=False)
    return hm, names + ("pad",) * len(pad)


@functools.lru_cache(maxsize=None)
def max_preds_nan_case(H, W):
    """(hm with NaNs [1,4,H,W], the same maps with every NaN replaced by -3e38).  What the kernel promises about NaN: it is never
    the arg-max, and a map of nothing but NaN gives idx 0 and coords (0, 0).  Map 0: NaN at the first and last element and spread
    over the map, a finite peak on the top border (no nudge: no NaN meets one); map 1: NaN everywhere but one positive element;
    map 2: all NaN; map 3: no NaN."""
    HW = H * W
    hm = synth.uniform(74, f"mp.nan.{H}x{W}", (1, 4, H, W), -1.0, -0.5).numpy().copy()
    flat = hm.reshape(4, HW)
    flat[0, ::3] = np.nan
    flat[0, HW - 1] = np.nan
    flat[0, W // 2] = PEAK
    flat[1, :] = np.nan
    flat[1, HW - 2] = 0.5
    flat[2, :] = np.nan
    flat[3, HW // 3] = PEAK
    filled = np.where(np.isnan(hm), np.float32(-3e38), hm)
    return hm, filled


# ---- ft_heatmap_argmax_screen / ft_heatmap_min_margin: case table -----------------------------------------------------------------
SCREEN_REL = 0.0156
# (K, H, W, byte offset of the base pointer from a 16-byte boundary)
SCREEN_SHAPES = [(1, 1, 2, 0), (3, 7, 9, 0), (5, 33, 31, 0), (4, 2, 4, 0), (17, 8, 6, 0), (2, 16, 16, 0), (6, 4, 582, 0),
                 (17, 64, 48, 0), (17, 96, 72, 0), (256, 4, 4, 0), (17, 64, 48, 4)]
SCREEN_FINITE_KINDS = ["clean", "tie", "near_tie", "safe_margin", "max_near_zero", "all_negative"]
SCREEN_KINDS = SCREEN_FINITE_KINDS + [f"{v}_{w}" for v in ("nan", "posinf", "neginf") for w in ("first", "last", "tail")] + ["clean_again"]
# which of the finite kinds the header's rule flags (for K >= 2; the two-pixel shape is stated in screen_case)
SCREEN_FLAGGED_KINDS = {"tie", "near_tie", "max_near_zero"}


def screen_takes_vector_path(H, W, offset):
    return (H * W) % 4 == 0 and offset % 16 == 0


def _pair_positions(pattern, k, HW, vec):
    """Pixels of a map's (top-1, top-2).  The kernel gives a map to one wave; on the 16-byte path lane l reads vectors
    l, l + 64, ... (eight per trip of 512), on the scalar path elements l, l + 64, ..."""
    unit = 4 if vec else 1
    n = HW // unit
    if pattern == "vec" and HW >= 4:                                  # both inside one float4
        a = 4 * ((7 * k + 1) % (HW // 4))
        return a + 1, a + 2
    if pattern == "lane":                                             # one lane, different trips (or groups of a trip, in a short map)
        lane = (5 * k + 3) % 64
        step = 512 if n > 512 + lane else 64
        if lane + step < n:
            return unit * (lane + step), unit * lane + (unit - 1)
    if pattern == "ends" and HW >= 2:
        return HW - 1, 0
    p1 = (13 * k + 5) % HW                                            # different lanes
    p2 = (p1 + 1 + HW // 2) % HW
    return p1, p2 if p2 != p1 else (p1 + 1) % HW


@functools.lru_cache(maxsize=None)
def screen_case(K, H, W, offset):
    """(hm float32 [N,K,H,W], kinds): one crop per entry of SCREEN_KINDS.  Every map has a planted top-1 / top-2 pair over a
    background in [-0.9, -0.6): top-1 in [1, 1.37), top-2 half a unit below; the pair's pixels cycle through one float4 / one lane
    in two trips / two lanes / first and last element.  Map K - 1 holds the crop's largest value (~3), map 0 its smallest (~-1), so
    R ~ 4 spans maps owned by different waves, E = SCREEN_REL * R ~ 0.063.  The kind's own plant goes to one map (its wave varies
    with the kind): an exact tie; a margin of 0.06 < 2 E; a margin of 0.25 > 2 E; a top-1 of 0.03 < E; an all-negative map with
    top-1 -0.25; a NaN / +inf / -inf at a map's first element, last element, or in the ragged tail of the lane walk.
    The two-pixel shape (1, 1, 2) has no room for that: its crops are the pairs themselves."""
    HW = H * W
    vec = screen_takes_vector_path(H, W, offset)
    tag = f"scr.{K}.{H}.{W}.{offset}"
    nonfinite = {"nan": np.nan, "posinf": np.inf, "neginf": -np.inf}
    crops = []
    for ci, kind in enumerate(SCREEN_KINDS):
        base = kind.split("_")[0] if kind.split("_")[0] in nonfinite else kind
        if HW == 2:
            pair = {"clean": (1.0, 0.5), "tie": (1.0, 1.0), "near_tie": (0.5, 0.4375), "safe_margin": (0.75, 0.5),
                    "max_near_zero": (2.0 ** -8, -1.0), "all_negative": (-0.25, -0.5), "clean_again": (0.5, 2.0)}.get(base, (1.0, 0.5))
            crop = np.tile(np.array(pair, dtype=np.float32), (K, 1))
        else:
            crop = synth.uniform(81, f"{tag}.bg.{ci}", (K, HW), -0.9, -0.6).numpy().copy()
            u = synth.uniform01(82, f"{tag}.u.{ci}", (K + 2,))
            kp = ci % (K - 1) if K >= 2 else 0
            for k in range(K):
                p1, p2 = _pair_positions(("vec", "lane", "lanes", "ends")[(k + ci) % 4], k, HW, vec)
                t1 = np.float32(1.0 + 0.37 * u[k])
                t2 = t1 - np.float32(0.5)
                if K >= 2 and k == K - 1:
                    t1 = np.float32(3.0 + 0.05 * u[K])
                    t2 = t1 - np.float32(0.5)
                elif k == kp:
                    if kind == "tie":
                        t2 = t1
                    elif kind == "near_tie":
                        t2 = t1 - np.float32(0.06)
                    elif kind == "safe_margin":
                        t2 = t1 - np.float32(0.25)
                    elif kind == "max_near_zero":
                        t1, t2 = np.float32(0.03), np.float32(-0.47)
                    elif kind == "all_negative":
                        t1, t2 = np.float32(-0.25), np.float32(-0.5)
                crop[k, p1], crop[k, p2] = t1, t2
                if k == 0:
                    pmin = next(p for p in ((11 * ci + 3 + j) % HW for j in range(HW)) if p not in (p1, p2))
                    crop[0, pmin] = np.float32(-1.0 - 0.05 * u[K + 1])
        if base in nonfinite:
            where = kind.split("_")[1]
            unit = 4 if vec else 1
            n = HW // unit
            v = (n // 64) * 64 if n % 64 else max(n - 2, 0)
            k, p = {"first": (0, 0), "last": (K - 1, HW - 1), "tail": (K // 2, min(unit * v + unit - 1, HW - 1))}[where]
            crop[k, p] = nonfinite[base]
        crops.append(crop.reshape(K, H, W))
    hm = np.ascontiguousarray(np.stack(crops), dtype=np.float32)
    hm.setflags(write=False)
    return hm, tuple(SCREEN_KINDS)


def selective_screen_input():
    """The synthetic input of tests/test_pose_gpu.py::test_argmax_screen_is_selective, restated: 40 crops of 17 single-peak
    maps, of which it plants a near-tie (crop 3), a maximum at 5e-4 < E (7), a NaN (11) and an Inf (13).  -> (hm, rel, special)"""
    N, K, H, W = 40, 17, 64, 48
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cy = (4 + (synth.uniform01(91, "cy", (N, K)) * (H - 8))).astype(np.int64)
    cx = (4 + (synth.uniform01(91, "cx", (N, K)) * (W - 8))).astype(np.int64)
    amp = torch.from_numpy(0.7 + 0.3 * synth.uniform01(91, "amp", (N, K)).astype(np.float32))
    hm = amp[..., None, None] * torch.exp(-((yy - torch.from_numpy(cy)[..., None, None]) ** 2 + (xx - torch.from_numpy(cx)[..., None, None]) ** 2) / 8.0)
    hm = (hm + 1e-3 * synth.normal(91, "noise", (N, K, H, W))).contiguous()
    hm[3, 2, cy[3, 2], cx[3, 2] + 1] = hm[3, 2, cy[3, 2], cx[3, 2]] - 1e-3
    hm[7, 5] = hm[7, 5] - hm[7, 5].max() + 5e-4
    hm[11, 0, 1, 1] = float("nan")
    hm[13, 16, 2, 2] = float("inf")
    return hm.numpy(), 1.6e-3, (3, 7, 11, 13)


# ---- ft_gather_flagged_rows: case table -------------------------------------------------------------------------------------------
GATHER_NS = [1, 3, 5, 255, 256, 257, 1023, 1024]
GATHER_ROW_REAL = 3 * 256 * 192 * 4           # a crop of the pose net's input: the row the exact mode gathers
GATHER_ROW_CAPPED = 4 * 1024 * 1024 + 48      # more than 64 pieces of 256 x 16 x 16 bytes: grid.y is capped, every block strides


def gather_patterns(N):
    """name -> int32 flags [N].  The kernel gives flags 4 t .. 4 t + 3 to thread t: rows >= 256 belong to waves 1..3."""
    half = (synth.uniform01(95, f"gather.half.{N}", (N,)) < 0.5).astype(np.int32)
    rows = np.arange(N)
    pats = {"none": np.zeros(N, np.int32), "all": np.ones(N, np.int32), "first": (rows == 0).astype(np.int32),
            "last": (rows == N - 1).astype(np.int32), "rows_ge_256": (rows >= 256).astype(np.int32),
            "rows_ge_768": (rows >= 768).astype(np.int32), "half": half, "half_value_7": half * 7, "half_value_minus_1": -half}
    return pats


# ---- ft_bn_batch_stats: case table ----------------------------------------------------------------------------------------------
# (N, H, W, C, cstride)
BN_EXACT_SHAPES = [(1, 1, 3, 8, 8), (1, 3, 3, 8, 32), (3, 17, 13, 72, 96), (2, 5, 7, 264, 264), (1, 4, 4, 512, 512), (3, 210, 210, 8, 8)]
BN_IMPULSE_SHAPE = (3, 17, 13, 72, 96)
BN_RANDOM_SHAPES = [(3, 17, 13, 72, 96), (2, 5, 7, 264, 264)]
BN_GUARD = 1.0e4                              # fills channels [C, cstride): must not leak into any statistic


def _bn_buffer(values, cstride):
    N, H, W, C = values.shape
    buf = np.full((N, H, W, cstride), BN_GUARD, dtype=np.float32)
    buf[..., :C] = values
    return buf


@functools.lru_cache(maxsize=None)
def bn_exact_input(shape):
    """Values from {0, 1, 2, 3} (exact in fp16 too): every sum of x and x^2 is an integer below 2^24, so fp32 sums are exact in
    any order.  -> float32 [N,H,W,cstride] with the guard channels filled."""
    N, H, W, C, cs = shape
    assert 9 * N * H * W < 2 ** 24
    return _bn_buffer(np.floor(synth.uniform01(97, f"bn.exact.{shape}", (N, H, W, C)) * 4.0).astype(np.float32), cs)


@functools.lru_cache(maxsize=None)
def bn_impulse_input():
    """Channel c is zero but for 1.0 at pixel p_c: p = 0, 7, 8, npix - 1, then a seeded spread.  -> (buffer, p int64 [C])"""
    N, H, W, C, cs = BN_IMPULSE_SHAPE
    npix = N * H * W
    p = np.floor(synth.uniform01(98, "bn.impulse", (C,)) * npix).astype(np.int64)
    p[:4] = (0, 7, 8, npix - 1)
    values = np.zeros((npix, C), dtype=np.float32)
    values[p, np.arange(C)] = 1.0
    return _bn_buffer(values.reshape(N, H, W, C), cs), p


@functools.lru_cache(maxsize=None)
def bn_random_input(shape, fp16):
    N, H, W, C, cs = shape
    x = synth.normal(99, f"bn.random.{shape}", (N, H, W, C), std=2.0, mean=0.7)
    if fp16:
        x = x.half().float()
    return _bn_buffer(x.numpy(), cs)


# ---- ft_crop_affine_fwd: one batch past the grid cap --------------------------------------------------------------------------------
CROP_RES = (256, 192)
CROP_BOXES = 90                               # 90 x 256 x 192 = 4 423 680 output pixels; the launch is capped at 16384 x 256 = 4 194 304
CROP_CHECKED = (0, 84, 85, 86, 89)            # the second grid-stride trip starts inside box 85


@functools.lru_cache(maxsize=None)
def crop_case():
    """(img uint8 [120,160,3], boxes float32 [90,3] = (centre x, centre y, scale))."""
    H, W = 120, 160
    img = (synth.uniform01(2, "kp.crop.img", (H, W, 3)) * 255).astype(np.uint8)
    u = synth.uniform01(3, "kp.crop.boxes", (CROP_BOXES, 3))
    boxes = np.stack((-10.0 + u[:, 0] * (W + 20.0), -10.0 + u[:, 1] * (H + 20.0), 60.0 + u[:, 2] * 240.0), axis=1).astype(np.float32)
    assert CROP_BOXES * CROP_RES[0] * CROP_RES[1] > 16384 * 256 > 85 * CROP_RES[0] * CROP_RES[1]
    assert 16384 * 256 < 86 * CROP_RES[0] * CROP_RES[1]
    return img, boxes
