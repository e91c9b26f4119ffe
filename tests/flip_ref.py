"""CPU references and seeded case tables for the flip test's two kernels: ft_hflip_nchw_f32 (the mirrored input) and
ft_heatmap_flip_merge (merged = (hm + mirrored, left/right-swapped hm_flip) * 0.5 and the key points of `merged`).  TEST
INFRASTRUCTURE ONLY: plain numpy, float32 exactly where the kernel rounds (one add, one multiply by 0.5), float64 selections through
keypoint_ref.max_preds_ref64, no GPU.  tests/test_flip_cpu.py pins every reference and case here (to tools.pose.main._flip_back and to
answers known by construction) before tests/test_flip_gpu.py judges the kernels with them.

A case is (hm, hm_flip, perm): hm_flip is what the net would give for the MIRRORED crop, i.e. in the mirrored frame and with the left/right
channels not yet swapped back.  Cases are built in the merged frame first (a second map `b` that lines up with hm pixel for pixel
and channel for channel) and then taken back with unflip(): hm_flip[:, perm[k]] = b[:, k] mirrored."""
import functools

import numpy as np

import keypoint_ref as R
from flowtrack.pytorch_amd import synth

HALF = np.float32(0.5)
COCO_PAIRS = ((2, 1), (4, 3), (6, 5), (8, 7), (10, 9), (12, 11), (14, 13), (16, 15))      # tools/pose/main.FLIP_PAIRS, restated
MPII_PAIRS = ((0, 5), (1, 4), (2, 3), (10, 15), (11, 14), (12, 13))


# ---- references -------------------------------------------------------------------------------------------------------------
def hflip_ref(x):
    """y[..., w] = x[..., W - 1 - w]."""
    return np.array(np.asarray(x)[..., ::-1], order="C", copy=True)


def perm_from_pairs(pairs, K):
    """Channel permutation of a pair table: perm[a] = b and perm[b] = a, every other joint fixed."""
    perm = list(range(K))
    for a, b in pairs:
        perm[a], perm[b] = b, a
    return tuple(perm)


def effective_perm(perm, K):
    """What the kernel reads: None = identity, an entry outside [0, K) = the map's own index."""
    if perm is None:
        return tuple(range(K))
    assert len(perm) == K
    return tuple(int(p) if 0 <= int(p) < K else k for k, p in enumerate(perm))


def flip_merge_ref(hm, hm_flip, perm):
    """(hm + hm_flip[:, perm][..., ::-1]) * float32(0.5) in float32: exactly two roundings per element."""
    hm, hm_flip = np.asarray(hm), np.asarray(hm_flip)
    assert hm.dtype == np.float32 and hm_flip.dtype == np.float32 and hm.shape == hm_flip.shape and hm.ndim == 4
    back = hm_flip[:, list(effective_perm(perm, hm.shape[1]))][..., ::-1]
    with np.errstate(invalid="ignore"):
        s = hm + back
        out = s * HALF
    assert s.dtype == np.float32 and out.dtype == np.float32
    return np.ascontiguousarray(out)


def flip_keypoints_ref(hm, hm_flip, perm, adjust):
    """max_preds_ref64 of the merged maps -> (merged, idx int32 [N,K], rows float32 [N,K,3] = x, y, score)."""
    merged = flip_merge_ref(hm, hm_flip, perm)
    idx, score, coords = R.max_preds_ref64(merged, adjust)
    return merged, idx, np.concatenate((coords, score[..., None]), axis=2).astype(np.float32)


def unflip(b, perm):
    """The hm_flip whose mirrored, permuted view is `b`: hm_flip[:, perm[k]] = b[:, k][..., ::-1] (perm a permutation)."""
    b = np.asarray(b)
    p = list(effective_perm(perm, b.shape[1]))
    assert sorted(p) == list(range(b.shape[1]))
    out = np.empty_like(b)
    out[:, p] = b[..., ::-1]
    return np.ascontiguousarray(out)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def adjacent_pairs_perm(K):
    """(0 1)(2 3)...: every joint but the last of an odd K changes place."""
    return perm_from_pairs([(k, k + 1) for k in range(0, K - 1, 2)], K)


# ---- ft_hflip_nchw_f32 ----------------------------------------------------------------------------------------------------------
# (N, C, H, W, byte offset of both pointers from a 16-byte boundary).  The last one takes the scalar path through its pointers alone.
HFLIP_SHAPES = [(1, 1, 1, 1, 0), (2, 3, 5, 7, 0), (1, 3, 32, 32, 0), (3, 3, 64, 48, 0), (2, 3, 8, 8, 4)]
# the grid is capped at 8192 blocks x 256 threads = 2 097 152 threads, one 16-byte group (or one element, on the scalar path) each:
# 2 211 840 groups of 4 / 2 099 196 elements of an odd width need a second grid-stride trip
HFLIP_SECOND_TRIP = [(6, 3, 768, 640, 0), (3, 1, 836, 837, 0)]
assert 6 * 3 * 768 * 640 // 4 > 8192 * 256 and 3 * 836 * 837 > 8192 * 256


@functools.lru_cache(maxsize=None)
def hflip_input(shape):
    N, C, H, W, _ = shape
    x = synth.normal(61, f"flip.hflip.{shape}", (N, C, H, W)).numpy().copy()
    return _frozen(x)[0]


# ---- ft_heatmap_flip_merge: planted cases -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_case(H, W, layout):
    """hm = the planted maps M of keypoint_ref.max_preds_case, hm_flip = M taken back through the mirror and a pair-swapping
    permutation: merged == M bit for bit (x + x and the halving are exact, subnormals included), so every plant keeps its
    property.  -> (hm, hm_flip, perm, names)"""
    M, names = R.max_preds_case(H, W, layout)
    perm = adjacent_pairs_perm(M.shape[1])
    return _frozen(np.array(M), unflip(M, perm)) + (perm, names)


@functools.lru_cache(maxsize=None)
def nan_case(H, W):
    """keypoint_ref.max_preds_nan_case built like the planted cases.  -> (hm, hm_flip, perm, filled): merged has a NaN exactly where
    hm has one, and its key points are those of `filled` for maps 0, 1, 3 (map 2, all NaN: idx 0 and coords (0, 0))."""
    M, filled = R.max_preds_nan_case(H, W)
    perm = adjacent_pairs_perm(M.shape[1])
    return _frozen(np.array(M), unflip(M, perm)) + (perm, filled)


# ---- ft_heatmap_flip_merge: what only the sum decides ----------------------------------------------------------------------------
SUM_SIZES = [(8, 6), (7, 9), (17, 19)]
SUM_KINDS = ("tie_by_merge", "max_in_neither_pass", "nudge_sign_flips", "max_exactly_zero")


@functools.lru_cache(maxsize=None)
def sum_case(H, W):
    """One crop of four maps, one per kind, over backgrounds in [-1, -0.5) in both passes (so is every merged background value).
    -> (hm, hm_flip, perm = None, info): info[kind] names the planted pixels (flat indices / (y, x)) the CPU test checks."""
    K, HW = len(SUM_KINDS), H * W
    a = synth.uniform(62, f"flip.sum.a.{H}x{W}", (1, K, H, W), -1.0, -0.5).numpy().copy()
    b = synth.uniform(62, f"flip.sum.b.{H}x{W}", (1, K, H, W), -1.0, -0.5).numpy().copy()
    fa, fb = a.reshape(K, HW), b.reshape(K, HW)
    info = {}
    # 1 + 3 at p and 3 + 1 at q > p: both merge to 2, the first one wins; alone, pass a picks q and pass b picks p
    p, q = HW // 3, HW - 2
    fa[0, p], fb[0, p], fa[0, q], fb[0, q] = 1.0, 3.0, 3.0, 1.0
    info["tie_by_merge"] = dict(p=p, q=q)
    # each pass has its own peak (2.0) where the other is at -1: merged 0.5; pixel c holds 1.5 in both: merged 1.5
    pa, pb, c = 1, HW - 3, HW // 2
    fa[1, pa], fb[1, pa], fa[1, pb], fb[1, pb], fa[1, c], fb[1, c] = 2.0, -1.0, -1.0, 2.0, 1.5, 1.5
    info["max_in_neither_pass"] = dict(pa=pa, pb=pb, c=c)
    # an interior peak whose neighbours say (-0.25, +0.25) in pass a alone and (+0.25, -0.25) after the merge
    y, x = H // 2, W // 2
    for m, (peak, left, right, up, down) in ((a, (2.0, 0.6, 0.3, 0.3, 0.6)), (b, (2.0, -0.9, 0.9, 0.9, -0.9))):
        m[0, 2, y, x], m[0, 2, y, x - 1], m[0, 2, y, x + 1], m[0, 2, y - 1, x], m[0, 2, y + 1, x] = peak, left, right, up, down
    info["nudge_sign_flips"] = dict(y=y, x=x)
    # +1 and -1 at one pixel: the merged maximum is exactly 0, so max_preds zeroes the coordinates
    z = HW // 2 + 1
    fa[3, z], fb[3, z] = 1.0, -1.0
    info["max_exactly_zero"] = dict(z=z)
    return _frozen(a, unflip(b, None)) + (None, info)


# ---- ft_heatmap_flip_merge: permutations ----------------------------------------------------------------------------------------
# name -> (N, K, H, W, perm).  The largest shape of the suite is the COCO one: 2 x 17 x 96 x 72
PERM_CASES = {
    "coco17_96x72": (2, 17, 96, 72, perm_from_pairs(COCO_PAIRS, 17)),
    "coco17_7x9": (2, 17, 7, 9, perm_from_pairs(COCO_PAIRS, 17)),
    "mpii16_64x48": (1, 16, 64, 48, perm_from_pairs(MPII_PAIRS, 16)),
    "k5_one_pair_8x6": (2, 5, 8, 6, perm_from_pairs(((1, 3),), 5)),
    "k1_9x1": (3, 1, 9, 1, (0,)),
    "k1_null_perm_1x7": (2, 1, 1, 7, None),
    "k3_out_of_range_17x19": (2, 3, 17, 19, (2, 7, 0)),            # entry 1 reads as itself
    "k3_negative_entry_8x6": (2, 3, 8, 6, (1, 0, -1)),
}


@functools.lru_cache(maxsize=None)
def perm_case(name):
    """Noise of std 0.25 around a constant of its own per map: 4 (k + 1) + 100 n in hm, 1000 + 8 (k + 1) + 300 n in hm_flip, so
    a merged map's mean names the two channels (and crops) it was made of.  -> (hm, hm_flip, perm)"""
    N, K, H, W, perm = PERM_CASES[name]
    hm = synth.normal(63, f"flip.perm.a.{name}", (N, K, H, W), std=0.25).numpy().copy()
    hf = synth.normal(63, f"flip.perm.b.{name}", (N, K, H, W), std=0.25).numpy().copy()
    for n in range(N):
        for k in range(K):
            hm[n, k] += np.float32(4 * (k + 1) + 100 * n)
            hf[n, k] += np.float32(1000 + 8 * (k + 1) + 300 * n)
    return _frozen(hm, hf) + (perm,)
