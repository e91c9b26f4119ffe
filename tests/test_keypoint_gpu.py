"""The pose-side helper kernels, each launched alone through the C ABI on torch-allocated buffers (a sentinel around every output)
and compared with the references and seeded case tables of tests/keypoint_ref.py, which tests/test_keypoint_cpu.py pins:
heat maps -> key points (ft_heatmap_max_preds, ft_heatmap_keypoint_rows), the arg-max screen of the exact mode
(ft_heatmap_argmax_screen, ft_heatmap_min_margin), the device-side compaction of its re-run set (ft_gather_flagged_rows), the
BatchNorm batch statistics (ft_bn_batch_stats) and one ft_crop_affine_fwd batch past the grid cap.  Shapes are the smallest that
reach every path of each kernel: maps below one wave, of exactly one block trip, with a partial second trip; ties whose smaller
index sits in the higher lane / the higher wave; the screen's scalar and 16-byte paths with ragged tails; flags owned by every
wave; channel counts past one trip of the channel-vector loop.  Three cases are large because only size reaches the path: a row
past 4 MiB (ft_gather_flagged_rows caps its grid), 132 300 pixels (ft_bn_batch_stats caps its grid) and 90 crops of 256 x 192
(ft_crop_affine_fwd's second grid-stride trip).

EXACT (torch.equal, scores and statistics bit for bit):
  ft_heatmap_max_preds / ft_heatmap_keypoint_rows   idx, score, coords (small integers +- 0.25); the rows layout
  ft_heatmap_argmax_screen                          flags; the four statistics of every crop without a non-finite value (each
                                                    is ONE IEEE float32 operation on selected values)
  ft_heatmap_min_margin                             the first of those statistics
  ft_gather_flagged_rows                            header, rows, everything behind them
BOUNDED, from the number formats alone:
  ft_bn_batch_stats, counts (values 0..3: every fp32 sum is an exact integer)  |mean err| <= 2^-22 |mean|,
        |var err| <= 2^-21 (mean(x^2) + mean^2): three roundings of 2^-24, doubled
  ft_bn_batch_stats, impulse    mean = 1 / npix to 2 ulp
  ft_bn_batch_stats, random     |mean err| <= (n - 1) 2^-24 mean|x| (n addends in ANY order),
        |var err| <= (n + 1) 2^-24 mean(x^2) + 2 |mean| mean_bound + mean_bound^2 + 2^-23 (mean(x^2) + mean^2)
  ft_crop_affine_fwd            0.05 grey level against the float64 crop, the bar of test_crop_kernel_matches_oracle
Worst err / bound of the random BN cases measured on an MI355X (every case prints its own; the order of the atomic adds moves
the last digit from run to run):
  (3, 17, 13, 72, 96)   fp32 mean 0.002 var 0.002   fp16 mean 0.002 var 0.004
  (2, 5, 7, 264, 264)   fp32 mean 0.019 var 0.029   fp16 mean 0.014 var 0.034
  (the count cases: mean <= 0.29, var <= 0.13 of their bounds; the impulses: 0.23 ulp; the crop: <= 1.8e-3 grey levels)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import keypoint_ref as R
from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd._lib import check
from oracle import tracking_ref

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
ISENTINEL = -7
GUARD = 4                                    # elements in front of and behind every output: 16 bytes, so alignment is kept
SIZES = pytest.mark.parametrize("size", R.MAX_PREDS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(n, dtype=torch.float32):
    """(whole buffer, the n elements a call may write): the sentinel everywhere, GUARD elements on each side."""
    buf = torch.full((n + 2 * GUARD,), ISENTINEL if dtype == torch.int32 else SENTINEL, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(*bufs):
    for buf in bufs:
        fill = ISENTINEL if buf.dtype == torch.int32 else SENTINEL
        if not (bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())):
            return False
    return True


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- ft_heatmap_max_preds / ft_heatmap_keypoint_rows --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _max_preds_want(H, W, layout, adjust):
    hm, _ = R.max_preds_case(H, W, layout)
    return tuple(torch.from_numpy(a) for a in R.max_preds_ref64(hm, adjust))


def _run_max_preds(hip_lib, hm, adjust):
    N, K, H, W = hm.shape
    g = torch.from_numpy(np.array(hm)).cuda()
    (bi, idx), (bs, score), (bc, coords) = _out(N * K, torch.int32), _out(N * K), _out(N * K * 2)
    check(hip_lib.ft_heatmap_max_preds(g.data_ptr(), N, K, H, W, adjust, idx.data_ptr(), score.data_ptr(), coords.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bi, bs, bc), "ft_heatmap_max_preds wrote outside its outputs"
    return idx.cpu().view(N, K), score.cpu().view(N, K), coords.cpu().view(N, K, 2)


def _run_keypoint_rows(hip_lib, hm, adjust):
    N, K, H, W = hm.shape
    g = torch.from_numpy(np.array(hm)).cuda()
    (bi, idx), (br, rows) = _out(N * K, torch.int32), _out(N * K * 3)
    check(hip_lib.ft_heatmap_keypoint_rows(g.data_ptr(), N, K, H, W, adjust, idx.data_ptr(), rows.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bi, br), "ft_heatmap_keypoint_rows wrote behind rows[N*K*3] or idx[N*K]"
    return idx.cpu().view(N, K), rows.cpu().view(N, K, 3)


def _assert_key_points(got, want, names, what):
    idx, score, coords = got
    w_idx, w_score, w_coords = want
    bad = (idx != w_idx) | (_bits(score) != _bits(w_score)) | (coords != w_coords).any(dim=2)
    if bool(bad.any()):
        n, k = (int(v) for v in bad.nonzero()[0])
        m = n * idx.shape[1] + k
        raise AssertionError(f"{what}: {int(bad.sum())} maps differ, first map ({n}, {k}) '{names[m]}': idx {int(idx[n, k])} want {int(w_idx[n, k])}, "
                             f"score {float(score[n, k])!r} want {float(w_score[n, k])!r}, coords {coords[n, k].tolist()} want {w_coords[n, k].tolist()}")
    assert torch.equal(idx, w_idx) and torch.equal(coords, w_coords) and torch.equal(_bits(score), _bits(w_score))


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("layout", R.MAX_PREDS_LAYOUTS)
@SIZES
def test_heatmap_max_preds(hip_lib, size, layout, adjust):
    """idx, score and coords of every planted map (keypoint_ref.max_preds_plants: ties inside one thread, across lanes, across
    waves with the smaller index in the higher one, first / last element, three-way, an all-equal map; a maximum of 0.0, -0.0 and
    the smallest subnormal against the `score > 0` mask; nudges with equal neighbours, one pixel inside each border, and none on
    the border) equal max_preds_ref64 exactly, as N x 1, N x 5 and 2 x K launches."""
    H, W = size
    hm, names = R.max_preds_case(H, W, layout)
    got = _run_max_preds(hip_lib, hm, adjust)
    _assert_key_points(got, _max_preds_want(H, W, layout, adjust), names, f"max_preds {H}x{W} {layout} adjust {adjust}")
    # a batch-index slip would repeat crop 0's answer (tests/test_keypoint_cpu.py: the two differ in the reference)
    assert not (torch.equal(got[0][0], got[0][1]) and torch.equal(got[1][0], got[1][1]))


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("layout", R.MAX_PREDS_LAYOUTS)
@SIZES
def test_heatmap_keypoint_rows(hip_lib, size, layout, adjust):
    """The same launch writing rows (x, y, score) with stride 3: bit for bit the three outputs of ft_heatmap_max_preds (and so
    the reference), idx equal, nothing written behind rows[N*K*3] and idx[N*K]."""
    H, W = size
    hm, names = R.max_preds_case(H, W, layout)
    idx, rows = _run_keypoint_rows(hip_lib, hm, adjust)
    m_idx, m_score, m_coords = _run_max_preds(hip_lib, hm, adjust)
    assert torch.equal(idx, m_idx)
    assert torch.equal(_bits(rows[..., :2]), _bits(m_coords)) and torch.equal(_bits(rows[..., 2]), _bits(m_score))
    _assert_key_points((idx, rows[..., 2], rows[..., :2]), _max_preds_want(H, W, layout, adjust), names, f"keypoint_rows {H}x{W} {layout} adjust {adjust}")


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("size", R.MAX_PREDS_SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_heatmap_max_preds_never_picks_a_nan(hip_lib, size, adjust):
    """What the header promises about NaN and no more: a NaN is never the arg-max (the answer is that of the map with every NaN
    replaced by a very negative number; no NaN sits beside a peak that gets a nudge), and a map of nothing but NaN gives idx 0
    and coords (0, 0)."""
    hm, filled = R.max_preds_nan_case(*size)
    idx, score, coords = _run_max_preds(hip_lib, hm, adjust)
    w_idx, w_score, w_coords = (torch.from_numpy(a) for a in R.max_preds_ref64(filled, adjust))
    keep = [0, 1, 3]
    assert torch.equal(idx[0, keep], w_idx[0, keep]) and torch.equal(score[0, keep], w_score[0, keep]) and torch.equal(coords[0, keep], w_coords[0, keep])
    assert int(idx[0, 2]) == 0 and coords[0, 2].tolist() == [0.0, 0.0]
    ridx, rows = _run_keypoint_rows(hip_lib, hm, adjust)
    assert torch.equal(ridx, idx) and torch.equal(rows[0, keep, :2], coords[0, keep]) and rows[0, 2, :2].tolist() == [0.0, 0.0]


# ---- ft_heatmap_argmax_screen / ft_heatmap_min_margin ----------------------------------------------------------------------------
def _run_screen(hip_lib, hm, offset, rel):
    N, K, H, W = hm.shape
    assert offset % 4 == 0
    buf = torch.full((hm.size + 2 * GUARD + offset // 4,), SENTINEL, dtype=torch.float32, device="cuda")
    first = GUARD + offset // 4
    buf[first:first + hm.size] = torch.from_numpy(np.array(hm)).flatten().cuda()
    ptr = buf.data_ptr() + 4 * first
    assert buf.data_ptr() % 16 == 0 and ptr % 16 == offset % 16
    (bf, flags), (bs, stats) = _out(N, torch.int32), _out(4 * N)
    check(hip_lib.ft_heatmap_argmax_screen(ptr, N, K, H, W, ctypes.c_float(rel), flags.data_ptr(), stats.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bf, bs), "ft_heatmap_argmax_screen wrote outside flags[N] / stats[N*4]"
    return flags.cpu().numpy(), stats.cpu().view(N, 4).numpy()


@pytest.mark.parametrize("shape", R.SCREEN_SHAPES, ids=str)
def test_heatmap_argmax_screen(hip_lib, shape):
    """Flags equal screen_ref; the statistics of every crop without a non-finite value equal its float32 statistics bit for bit —
    also those of the finite crops that share the launch with a NaN / +inf / -inf crop; of a non-finite crop only the flag.
    rel_bound = 0 flags only the non-finite crops.  The scalar path (HW % 4 != 0, or a base 4 bytes off a 16-byte boundary) and
    the 16-byte path with n4 = 2, 12, 64, 582 (a tail inside the second trip), 768, 1728; K from 1 to 256."""
    K, H, W, offset = shape
    hm, kinds = R.screen_case(*shape)
    for rel in (R.SCREEN_REL, 0.0):
        w_flags, w_stats, finite, _ = R.screen_ref(hm, rel)
        flags, stats = _run_screen(hip_lib, hm, offset, rel)
        wrong = [kinds[n] for n in np.flatnonzero((flags != 0) != (w_flags != 0))]
        assert not wrong and set(np.unique(flags).tolist()) <= {0, 1}, f"screen {shape} rel {rel}: flags differ for crops {wrong}"
        same = (stats[finite].view(np.int32) == w_stats[finite].view(np.int32)).all(axis=1)
        assert same.all(), (f"screen {shape} rel {rel}: statistics differ for crops {[k for k, s in zip(np.array(kinds)[finite], same) if not s]}: "
                            f"got {stats[finite][~same][0].tolist()} want {w_stats[finite][~same][0].tolist()}")
        assert torch.equal(torch.from_numpy(stats[finite]), torch.from_numpy(w_stats[finite]))
        if rel == 0.0:
            assert np.array_equal(flags != 0, ~finite)


def test_heatmap_argmax_screen_refuses_what_it_cannot_do(hip_lib):
    hm = torch.zeros((2, 257, 2, 2), dtype=torch.float32, device="cuda")
    (bf, flags), (bs, stats) = _out(2, torch.int32), _out(8)
    call = lambda K, H, W, rel: hip_lib.ft_heatmap_argmax_screen(hm.data_ptr(), 2, K, H, W, ctypes.c_float(rel), flags.data_ptr(), stats.data_ptr(), _stream())
    assert call(257, 2, 2, 0.01) != 0                 # K > 256
    assert call(4, 1, 1, 0.01) != 0                   # H * W = 1: no second value
    assert call(4, 2, 2, -0.01) != 0                  # negative bound
    assert call(4, 2, 2, float("nan")) != 0           # NaN bound
    torch.cuda.synchronize()
    assert bool((bf == ISENTINEL).all()) and bool((bs == SENTINEL).all()), "a refused call wrote to its outputs"
    assert call(256, 2, 2, 0.01) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [s for s in R.SCREEN_SHAPES if s[3] == 0], ids=str)
def test_heatmap_min_margin(hip_lib, shape):
    """On the finite crops of every screen case (HW from 2 to 6912, the exact tie among them) the smallest top-1 / top-2 margin
    equals the first statistic of screen_ref bit for bit."""
    K, H, W, _ = shape
    hm, kinds = R.screen_case(*shape)
    _, w_stats, finite, _ = R.screen_ref(hm, R.SCREEN_REL)
    sub = np.ascontiguousarray(hm[finite])
    N = sub.shape[0]
    g = torch.from_numpy(sub).cuda()
    bo, out = _out(N)
    check(hip_lib.ft_heatmap_min_margin(g.data_ptr(), N, K, H, W, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    want = torch.from_numpy(w_stats[finite, 0].copy())
    assert _guards_intact(bo) and torch.equal(_bits(out.cpu()), _bits(want)), (out.cpu().tolist(), want.tolist())
    assert float(out[list(np.array(kinds)[finite]).index("tie")]) == 0.0


# ---- ft_gather_flagged_rows ---------------------------------------------------------------------------------------------------------
def _check_gather(hip_lib, flags, src, g_src, row_bytes, what):
    """One launch against gather_ref: header[0 .. count], the compacted rows, and the untouched sentinel behind both."""
    N = len(flags)
    w_hdr, w_rows = R.gather_ref(flags, src)
    count = int(w_hdr[0])
    words = row_bytes // 4
    cap = min(N, count + 1)                                # rows of dst: one more than the call may fill (N when everything is flagged)
    g_flags = torch.from_numpy(flags).cuda()
    (bh, hdr), (bd, dst) = _out(1 + N, torch.int32), _out(cap * words, torch.int32)
    check(hip_lib.ft_gather_flagged_rows(g_flags.data_ptr(), N, g_src.data_ptr(), ctypes.c_longlong(row_bytes), dst.data_ptr(), hdr.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert hdr[:1 + count].cpu().tolist() == w_hdr.tolist(), f"{what}: header {hdr[:min(1 + count, 12)].tolist()} want {w_hdr[:12].tolist()}"
    assert bool((hdr[1 + count:] == ISENTINEL).all()), f"{what}: header written behind its {count} entries"
    assert torch.equal(dst[:count * words].view(count, words), torch.from_numpy(w_rows).cuda().view(count, words)), f"{what}: rows differ"
    assert bool((dst[count * words:] == ISENTINEL).all()), f"{what}: dst written behind its {count} rows"
    assert _guards_intact(bh, bd), f"{what}: wrote outside header[1 + N] / dst"


@pytest.mark.parametrize("N", R.GATHER_NS)
def test_gather_flagged_rows(hip_lib, N):
    """16-byte rows, every flag pattern of keypoint_ref.gather_patterns: none, all, only the first / last row, only rows owned by
    waves 1..3, a random half, and flag values 7 and -1 (anything non-zero counts)."""
    src = np.arange(N * 4, dtype=np.int32).reshape(N, 4) + 1000
    g_src = torch.from_numpy(src).cuda()
    for name, flags in R.gather_patterns(N).items():
        _check_gather(hip_lib, flags, src, g_src, 16, f"gather N {N} {name}")


@pytest.mark.parametrize("case", [(5, R.GATHER_ROW_REAL, "all"), (5, R.GATHER_ROW_REAL, "half"), (257, R.GATHER_ROW_REAL, "rows_ge_256"),
                                  (3, R.GATHER_ROW_CAPPED, "all"), (3, R.GATHER_ROW_CAPPED, "last"), (3, R.GATHER_ROW_CAPPED, "none")], ids=str)
def test_gather_flagged_rows_of_real_size(hip_lib, case):
    """LARGE ON PURPOSE: the row the exact mode gathers (a 3 x 256 x 192 fp32 crop, 144 pieces of 4 KiB: grid.y = 36) and a row
    of 4 MiB + 48 bytes, the smallest round size past 64 pieces of 64 KiB, where grid.y is capped and the copy loop strides."""
    N, row_bytes, pattern = case
    words = row_bytes // 4
    src = np.arange(N * words, dtype=np.int32).reshape(N, words)
    _check_gather(hip_lib, R.gather_patterns(N)[pattern], src, torch.from_numpy(src).cuda(), row_bytes, f"gather {case}")


def test_gather_flagged_rows_refuses_what_it_cannot_do(hip_lib):
    flags = torch.ones(1025, dtype=torch.int32, device="cuda")
    src = torch.zeros(1025 * 8, dtype=torch.int32, device="cuda")
    (bh, hdr), (bd, dst) = _out(1026, torch.int32), _out(1025 * 8, torch.int32)
    call = lambda N, s, rb, d: hip_lib.ft_gather_flagged_rows(flags.data_ptr(), N, s, ctypes.c_longlong(rb), d, hdr.data_ptr(), _stream())
    assert call(1025, src.data_ptr(), 16, dst.data_ptr()) != 0          # N > 1024
    assert call(8, src.data_ptr(), 24, dst.data_ptr()) != 0             # row_bytes no multiple of 16
    assert call(8, src.data_ptr() + 8, 16, dst.data_ptr()) != 0         # src 8 bytes off
    assert call(8, src.data_ptr(), 16, dst.data_ptr() + 8) != 0         # dst 8 bytes off
    torch.cuda.synchronize()
    assert bool((bh == ISENTINEL).all()) and bool((bd == ISENTINEL).all()), "a refused call wrote to its outputs"


# ---- ft_bn_batch_stats --------------------------------------------------------------------------------------------------------------
def _run_bn(hip_lib, buf, C, dtype):
    """buf: float32 numpy [N,H,W,cstride] with the guard channels filled -> (mean, var) float64 numpy [C], (mean64, var64) of the
    values as stored in `dtype`."""
    N, H, W, cs = buf.shape
    x = torch.from_numpy(np.array(buf)).to("cuda", dtype)
    ws = torch.full((2 * C,), SENTINEL, dtype=torch.float32, device="cuda")      # the call zeroes it itself
    (bm, mean), (bv, var) = _out(C), _out(C)
    check(hip_lib.ft_bn_batch_stats(x.data_ptr(), N, H, W, C, cs, _lib.dtype_code(dtype), ws.data_ptr(), mean.data_ptr(), var.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bm, bv), "ft_bn_batch_stats wrote outside mean[C] / var[C]"
    return mean.cpu().double().numpy(), var.cpu().double().numpy(), R.bn_ref64(x[..., :C])


def _report(what, err, bound):
    ratio = err / bound
    c = int(np.argmax(ratio))
    print(f"{what}: worst err / bound {ratio[c]:.3f} (err {err[c]:.3e}, bound {bound[c]:.3e}, channel {c})")
    return ratio[c]


@DTYPES
@pytest.mark.parametrize("shape", R.BN_EXACT_SHAPES, ids=str)
def test_bn_batch_stats_of_counts(hip_lib, shape, dtype):
    """Values from {0, 1, 2, 3}: all fp32 sums are exact integers in any order, so only the three roundings behind them remain
    (1 / n, the product, the difference): |mean err| <= 2^-22 |mean|, |var err| <= 2^-21 (mean(x^2) + mean^2).  Fewer than 8
    pixels, C = 8, a second trip of the channel-vector loop with one live lane (C = 264) and two full ones (C = 512), and the
    capped grid with its stride (132 300 pixels); the guard channels [C, cstride) hold 1e4 and must not leak."""
    N, H, W, C, cs = shape
    mean, var, (m64, v64) = _run_bn(hip_lib, R.bn_exact_input(shape), C, dtype)
    r_m = _report(f"bn counts {shape} {dtype} mean", np.abs(mean - m64), 2.0 ** -22 * np.abs(m64) + 1e-300)
    r_v = _report(f"bn counts {shape} {dtype} var", np.abs(var - v64), 2.0 ** -21 * (v64 + 2 * m64 * m64) + 1e-300)
    assert r_m <= 1.0 and r_v <= 1.0


@DTYPES
def test_bn_batch_stats_of_impulses(hip_lib, dtype):
    """One 1.0 per channel at pixel p_c (0, 7, 8, npix - 1 and a seeded spread), zero elsewhere: a pixel that is skipped or
    counted twice shows in its own channel.  mean = 1 / npix to 2 ulp."""
    N, H, W, C, cs = R.BN_IMPULSE_SHAPE
    buf, p = R.bn_impulse_input()
    mean, var, (m64, v64) = _run_bn(hip_lib, buf, C, dtype)
    want = 1.0 / (N * H * W)
    ulp = float(np.spacing(np.float32(want)))
    err = np.abs(mean - want)
    print(f"bn impulses {dtype}: worst mean err {err.max() / ulp:.2f} ulp (pixel {int(p[int(np.argmax(err))])})")
    assert (err <= 2 * ulp).all(), f"channels {np.flatnonzero(err > 2 * ulp).tolist()}, pixels {p[err > 2 * ulp].tolist()}"
    assert np.abs(var - v64).max() <= 2.0 ** -21 * (want + want * want)


@DTYPES
@pytest.mark.parametrize("shape", R.BN_RANDOM_SHAPES, ids=str)
def test_bn_batch_stats_of_random_values(hip_lib, shape, dtype):
    """N(0.7, 2^2) values against float64 with the order-independent worst case of an fp32 sum of n addends."""
    N, H, W, C, cs = shape
    buf = R.bn_random_input(shape, dtype == torch.float16)
    mean, var, (m64, v64) = _run_bn(hip_lib, buf, C, dtype)
    n = N * H * W
    x = buf[..., :C].reshape(n, C).astype(np.float64)
    mabs, msq = np.abs(x).mean(axis=0), (x * x).mean(axis=0)
    b_mean = (n - 1) * 2.0 ** -24 * mabs
    b_var = (n + 1) * 2.0 ** -24 * msq + 2 * np.abs(m64) * b_mean + b_mean ** 2 + 2.0 ** -23 * (msq + m64 * m64)
    r_m = _report(f"bn random {shape} {dtype} mean", np.abs(mean - m64), b_mean)
    r_v = _report(f"bn random {shape} {dtype} var", np.abs(var - v64), b_var)
    assert r_m <= 1.0 and r_v <= 1.0


def test_bn_batch_stats_refuses_what_it_cannot_do(hip_lib):
    x = torch.zeros((1, 2, 2, 96), dtype=torch.float32, device="cuda")
    ws = torch.zeros(192, dtype=torch.float32, device="cuda")
    (bm, mean), (bv, var) = _out(96), _out(96)
    call = lambda C, cs: hip_lib.ft_bn_batch_stats(x.data_ptr(), 1, 2, 2, C, cs, _lib.FT_F32, ws.data_ptr(), mean.data_ptr(), var.data_ptr(), _stream())
    assert call(12, 16) != 0                          # C no multiple of 8
    assert call(16, 8) != 0                           # cstride below C
    assert call(72, 76) != 0                          # cstride no multiple of 8
    torch.cuda.synchronize()
    assert bool((bm == SENTINEL).all()) and bool((bv == SENTINEL).all()), "a refused call wrote to its outputs"


# ---- ft_crop_affine_fwd ---------------------------------------------------------------------------------------------------------------
def test_crop_affine_past_the_grid_cap(hip_lib):
    """LARGE ON PURPOSE: the launch is capped at 16384 workgroups of 256 threads = 4 194 304 output pixels per grid-stride trip;
    90 crops of 256 x 192 (what the multi-clip pipeline batches) are 4 423 680, so the second trip starts inside box 85.  Boxes
    0, 84, 85, 86 and 89 against the float64 crop of oracle/tracking_ref.py, un-normalised, to 0.05 grey level."""
    img, boxes = R.crop_case()
    rh, rw = R.CROP_RES
    nb, C = len(boxes), img.shape[2]
    g_img, g_boxes = torch.from_numpy(img).cuda(), torch.from_numpy(boxes).cuda()
    bo, out = _out(nb * C * rh * rw)
    check(hip_lib.ft_crop_affine_fwd(g_img.data_ptr(), img.shape[0], img.shape[1], C, g_boxes.data_ptr(), nb, rh, rw, None, None,
                                     ctypes.c_float(1.0), out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bo), "ft_crop_affine_fwd wrote outside its output"
    got = out.view(nb, C, rh, rw)
    assert not bool((got == SENTINEL).any()), "output pixels left unwritten"
    for b in R.CROP_CHECKED:
        want = tracking_ref.crop_affine_ref(img, boxes[b, :2].astype(np.float64), float(boxes[b, 2]), (rh, rw))
        err = float(np.abs(got[b].cpu().numpy().astype(np.float64) - want).max())
        print(f"crop_affine box {b}: max err {err:.3e} grey levels (bound 0.05)")
        assert err <= 0.05, f"box {b}"
