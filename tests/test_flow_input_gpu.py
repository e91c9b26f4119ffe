"""The flow input kernels (csrc/aux_ops.hip), each entry point launched alone through the C ABI and held BIT FOR BIT to the numpy
reference of tests/flow_input_ref.py:

  ft_flow_rgb_mean                             two partial-sum paths + the finish kernel
  ft_flow_pack_pair                            the scalar and the 4-pixel pack kernel
  ft_flow_pack_pair_sums + ft_flow_mean_fold   the fp16 default
  ft_flow_mean_pack_pair                       one launch, partial sums exchanged through tagged 8-byte words

The frames hold integers whose colour sums stay below 2^22, so every partial sum is an exact fp32 integer in any order, the mean
is one rounded product and a packed value one correctly rounded subtract, divide and cast (tests/test_flow_input_cpu.py checks
these properties of the inputs).  Every comparison is torch.equal on the values' BIT patterns (so -0 and +0 differ as well);
the only tolerance is ft_flow_mean_fold's shift_n (1e-5 against float64: that expression may be contracted to FMAs).

Every output buffer, partial-sum workspace, `mean` and `state` is a slice of a larger allocation with guard bands of at least
one view row / 256 elements on both sides; outputs start as NaN, so an element a kernel leaves out fails the comparison, and
the bands must come back untouched.

fp16 subnormals: where the mean lies within 0.0156 of a pixel value, (x - mean) / 255 is an fp16 subnormal.  The first frame set
alone puts 510 897 such elements into the fp16 references (291 at 13 x 512, 6 512 at 5 x 6144, 154 482 at 160 x 832, 349 612 at
42 x 6144; tests/test_flow_input_cpu.py keeps them there).  On an MI355X all of them come back bit-equal to numpy's
round-to-nearest-even: the kernels do NOT flush them, nothing is compared against a flushed value, and the reference network's
((x - mean) / rgb_max in fp32, then .half(), which rounds the same way) would not differ either.

Measured on an MI355X: every case of this module is exact as the kernels stand — no kernel or dispatch needed a fix.  Tried once
against a build broken on purpose (the mean's tail loop losing the last float4 of a split; the 4-pixel pack kernel multiplying
by 1 / rgb_max instead of dividing): 26 of the 99 cases failed — the mean cases of the six shapes whose last float4 falls into the
tail loop, every W % 4 == 0 pack case, both route comparisons — and the rest passed.
ft_flow_rgb_mean takes no rgb_max, so the rgb_max = 0 refusal and the rgb_max = 256 case cover the other four entry points."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flow_input_ref as R
from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_F16, FT_F32, check

pytestmark = pytest.mark.gpu
IDS = [R.sid(s) for s in R.SHAPES]
W4_SHAPES = [s for s in R.SHAPES if s[2] % 4 == 0]
FUSED_SHAPES = [s for s in R.SHAPES if R.fused_plan(s[1], s[2]) is not None]
MULTI_WG_SHAPES = [s for s in FUSED_SHAPES if R.fused_plan(s[1], s[2])[1] in (2, 3, 5, 23, 42)]
SMALL = (3, 25, 512)                        # the shape of the one-off cases (rgb_max 256, mutations, epoch wrap)
GUARD_F, GUARD_I = -1024.0, 0x5A5A5A5A5A5A5A5A
NP_OF = {torch.float16: np.float16, torch.float32: np.float32}
CODE_OF = {torch.float16: FT_F16, torch.float32: FT_F32}
LAYOUTS = ((0, 0), (3, 6), (1, 5))          # (lpad, wpitch - W)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """`shape` elements inside a larger allocation: guard bands before and after, the payload poisoned (NaN for floats)."""

    def __init__(self, shape, dtype, row_elems=0, poison=float("nan")):
        n = int(np.prod(shape))
        self.g = g = -(-max(256, row_elems) // 256) * 256
        self.guard = GUARD_F if dtype.is_floating_point else GUARD_I
        self.raw = torch.full((n + 2 * g,), self.guard, dtype=dtype, device="cuda")
        self.t = self.raw[g:g + n].view(shape)
        self.t.fill_(poison)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.g] == self.guard).all()) and bool((self.raw[self.g + self.n:] == self.guard).all())


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(got, want):
    """got: GPU tensor; want: numpy array or GPU tensor of the same shape and type.  True when every element has the same bits."""
    if isinstance(want, np.ndarray):
        want = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return torch.equal(_bits(got), _bits(want))


def _assert_bits(got, want, what):
    if _same_bits(got, want):
        return
    w = want if isinstance(want, np.ndarray) else want.cpu().numpy()
    g = got.cpu().numpy()
    u = {2: np.uint16, 4: np.uint32}[g.itemsize]
    bad = np.flatnonzero(np.ascontiguousarray(g).view(u).ravel() != np.ascontiguousarray(w).view(u).ravel())
    wb = w.ravel()[bad].astype(np.float64)
    sub = int(((np.abs(wb) < 2.0 ** -14) & (wb != 0)).sum()) if g.itemsize == 2 else 0
    i = int(bad[0])
    pytest.fail(f"{what}: {bad.size} of {g.size} elements differ ({sub} of them where the reference is an fp16 subnormal); first at "
                f"flat index {i} {np.unravel_index(i, g.shape)}: got {g.ravel()[i]!r}, want {w.ravel()[i]!r}; "
                f"got[bad][:8] {g.ravel()[bad[:8]]}, want[bad][:8] {w.ravel()[bad[:8]]}")


@functools.lru_cache(maxsize=16)
def _frames(rep, B, H, W):
    """(frames, expected mean): computed once, shared, never written to."""
    x = R.int_pairs(rep, B, H, W)
    return x, R.expected_mean(x)


# ---- one launch of each entry point, guards checked ------------------------------------------------------------------------
def _run_mean(hip_lib, gx, B, H, W):
    partial = Guarded((B * 3, R.SPLITS), torch.float32)
    mean = Guarded((B * 3,), torch.float32)
    check(hip_lib.ft_flow_rgb_mean(gx.data_ptr(), B, H, W, partial.ptr(), mean.ptr(), _stream()))
    torch.cuda.synchronize()
    assert partial.intact() and mean.intact()
    return partial.t, mean.t


def _check_mean(hip_lib, x, what):
    B, _, _, H, W = x.shape
    partial, mean = _run_mean(hip_lib, torch.from_numpy(x).cuda(), B, H, W)
    _assert_bits(mean, R.expected_mean(x), f"mean {what}")
    _assert_bits(partial, R.split_sums(x), f"partial {what}")
    return mean


def _run_pack(hip_lib, gx, gmean, rgb_max, B, H, W, mode, lpad, wpitch, dtype):
    shape = (B, H, wpitch, 8) if mode == 0 else (2 * B, H, wpitch, 4)
    y = Guarded(shape, dtype, row_elems=wpitch * shape[3])
    check(hip_lib.ft_flow_pack_pair(gx.data_ptr(), gmean.data_ptr(), rgb_max, y.ptr(), B, H, W, mode, lpad, wpitch, CODE_OF[dtype],
                                    _stream()))
    torch.cuda.synchronize()
    assert y.intact(), ("guard band written", B, H, W, mode, lpad, wpitch, dtype)
    return y.t


def _check_pack(hip_lib, x, gx, means, rgb_max, layouts=LAYOUTS, dtypes=(torch.float32, torch.float16)):
    """Every (dtype, mode, layout) of ft_flow_pack_pair on x with each of `means` (GPU tensors holding the expected mean)."""
    B, _, _, H, W = x.shape
    xn = R.normalise(x, R.expected_mean(x), rgb_max)
    for dtype in dtypes:
        for mode in (0, 1):
            for lpad, extra in layouts:
                wpitch = W + extra
                want = (R.view6 if mode == 0 else R.view3)(xn, lpad, wpitch, NP_OF[dtype])
                want_g = torch.from_numpy(want).cuda()
                for gmean in means:
                    got = _run_pack(hip_lib, gx, gmean, rgb_max, B, H, W, mode, lpad, wpitch, dtype)
                    assert got.numel() == want.size == (1 + mode) * B * H * wpitch * (8 >> mode)
                    _assert_bits(got, want_g, f"pack {B}x{H}x{W} {dtype} mode {mode} lpad {lpad} wpitch {wpitch}")


def _check_fold(hip_lib, x, rgb_max, configs=((3, 0), (1, 0), (3, 2), (1, 2)), what=""):
    """ft_flow_pack_pair_sums + ft_flow_mean_fold on x for each (pad, wpitch - W - 2 pad); returns the last mean."""
    B, _, _, H, W = x.shape
    gx = torch.from_numpy(x).cuda()
    mean_want = R.expected_mean(x)
    nchunk = int(hip_lib.ft_flow_pack_pair_sums_chunks(H))
    assert nchunk == R.fold_chunks(H)
    g = torch.Generator().manual_seed(5)
    wsum, scale, shift = torch.randn((64, 8), generator=g), torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    wsum_g, scale_g, shift_g = wsum.cuda(), scale.cuda(), shift.cuda()
    mean = None
    for pad, extra in configs:
        wpitch = W + 2 * pad + extra
        tag = f"fold {what} {B}x{H}x{W} pad {pad} wpitch {wpitch} rgb_max {rgb_max}"
        y = Guarded((B, H + 2 * pad, wpitch, 8), torch.float16, row_elems=wpitch * 8)
        partial = Guarded((B * 3, nchunk), torch.float32)
        check(hip_lib.ft_flow_pack_pair_sums(gx.data_ptr(), rgb_max, y.ptr(), B, H, W, pad, wpitch, FT_F16, partial.ptr(), _stream()))
        torch.cuda.synchronize()
        assert y.intact() and partial.intact(), tag
        _assert_bits(partial.t, R.chunk_sums(x), f"chunk sums, {tag}")
        want = torch.from_numpy(R.fold_view(x, mean_want, pad, wpitch, rgb_max)).cuda()
        inner = torch.zeros((H + 2 * pad, wpitch), dtype=torch.bool, device="cuda")
        inner[pad:pad + H, pad:pad + W] = True
        _assert_bits(y.t[:, inner], want[:, inner], f"inner pixels after pass 1, {tag}")
        assert bool(torch.isnan(y.t[:, ~inner]).all()), f"pass 1 wrote a padding pixel, {tag}"
        for use_scale in (True, False):
            for use_shift in (True, False):
                for cout in (64, 7):
                    shn = Guarded((B, cout), torch.float32)
                    mean = Guarded((B * 3,), torch.float32)
                    check(hip_lib.ft_flow_mean_fold(partial.ptr(), rgb_max, y.ptr(), B, H, W, pad, wpitch, FT_F16, wsum_g.data_ptr(),
                                                    scale_g.data_ptr() if use_scale else None,
                                                    shift_g.data_ptr() if use_shift else None, cout, shn.ptr(), mean.ptr(), _stream()))
                    torch.cuda.synchronize()
                    assert y.intact() and partial.intact() and shn.intact() and mean.intact(), tag
                    _assert_bits(mean.t, mean_want, f"mean, {tag}")
                    _assert_bits(y.t, want, f"padded view (inner: fp16(x / rgb_max), padding: fp16(mean / rgb_max)), {tag}")
                    want_shn = R.fold_shift(mean_want, wsum.numpy()[:cout], scale.numpy()[:cout] if use_scale else None,
                                            shift.numpy()[:cout] if use_shift else None, rgb_max)
                    err = np.abs(shn.t.cpu().numpy().astype(np.float64) - want_shn).max()
                    assert err <= 1e-5, (tag, use_scale, use_shift, cout, err)
    return mean.t


FUSED_L6, FUSED_L3 = (3, 6), (1, 5)         # (lpad, wpitch - W) of the 6-channel and of the siamese view: different on purpose
COMBOS = ((True, True), (True, False), (False, True))


def _fused_refs(x, rgb_max, dtype):
    W = x.shape[-1]
    xn = R.normalise(x, R.expected_mean(x), rgb_max)
    return (torch.from_numpy(R.view6(xn, FUSED_L6[0], W + FUSED_L6[1], NP_OF[dtype])).cuda(),
            torch.from_numpy(R.view3(xn, FUSED_L3[0], W + FUSED_L3[1], NP_OF[dtype])).cuda())


def _fused_launch(hip_lib, gx, B, H, W, rgb_max, dtype, state, use6=True, use3=True):
    """One launch on `state` (a Guarded int64 buffer); returns (y or None, y3 or None, mean) after the guard checks."""
    wp6, wp3 = W + FUSED_L6[1], W + FUSED_L3[1]
    y = Guarded((B, H, wp6, 8), dtype, row_elems=wp6 * 8) if use6 else None
    y3 = Guarded((2 * B, H, wp3, 4), dtype, row_elems=wp3 * 4) if use3 else None
    mean = Guarded((B * 3,), torch.float32)
    check(hip_lib.ft_flow_mean_pack_pair(gx.data_ptr(), rgb_max, y.ptr() if y else None, FUSED_L6[0], wp6, y3.ptr() if y3 else None,
                                         FUSED_L3[0], wp3, B, H, W, CODE_OF[dtype], state.ptr(), mean.ptr(), _stream()))
    torch.cuda.synchronize()
    assert int(state.t[-1]) == 0, "a workgroup timed out waiting for its sample's partial sums"
    assert state.intact() and mean.intact() and (y is None or y.intact()) and (y3 is None or y3.intact())
    return (y.t if y else None), (y3.t if y3 else None), mean.t


def _fused_state(hip_lib, B, H, W):
    words = int(hip_lib.ft_flow_mean_pack_pair_state_words(B, H, W))
    assert words == R.fused_state_words(B, H, W) > 0
    return Guarded((words,), torch.int64, poison=0)          # zeroed ONCE


def _check_fused(hip_lib, gx, shape, mean_want, refs, rgb_max, dtype, state, use6, use3, what):
    B, H, W = shape
    y, y3, mean = _fused_launch(hip_lib, gx, B, H, W, rgb_max, dtype, state, use6, use3)
    _assert_bits(mean, mean_want, f"mean, {what}")
    if use6:
        _assert_bits(y, refs[0], f"6-channel view, {what}")
    if use3:
        _assert_bits(y3, refs[1], f"siamese view, {what}")
    return y, y3, mean


# ---- (a) ft_flow_rgb_mean ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_rgb_mean_is_exact(hip_lib, shape):
    """mean == fp32(S) * fp32(1 / L) and every partial[bc * 64 + split] == the exact integer sum of its span (0 where empty)."""
    x, _ = _frames(0, *shape)
    _check_mean(hip_lib, x, R.sid(shape))


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_rgb_mean_impulses(hip_lib, shape):
    """One pixel per (sample, colour): first / last pixel of each frame, first / last element of splits 0, 1, 31, 63, and the
    elements on both sides of the tail loop's start at 160 x 832.  A span that starts or ends one element off loses it."""
    _, H, W = shape
    for launch in R.impulse_launches(H, W, R.mean_impulse_positions(H, W)):
        _check_mean(hip_lib, R.impulse_pairs(len(launch) // 3, H, W, launch), f"{H}x{W} impulses {launch}")


# ---- (b) ft_flow_pack_pair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_pack_pair_is_exact(hip_lib, shape):
    """fp32 and fp16, both modes, three layouts: live columns, zero pad columns and zero channels, all bit-equal; with the expected
    mean fed from the host and with the mean ft_flow_rgb_mean returned (odd W: the scalar kernel, else the 4-pixel one)."""
    B, H, W = shape
    x, mean = _frames(0, B, H, W)
    gx = torch.from_numpy(x).cuda()
    _, dev_mean = _run_mean(hip_lib, gx, B, H, W)
    _assert_bits(dev_mean, mean, "mean")
    _check_pack(hip_lib, x, gx, (torch.from_numpy(mean).cuda(), dev_mean), R.RGB_MAX)


@pytest.mark.parametrize("shape", [(2, 9, 40), SMALL], ids=R.sid)
def test_pack_pair_scalar_kernel_on_an_offset_pointer(hip_lib, shape):
    """W % 4 == 0 but the input only 4-byte aligned: the entry point's own check sends it to the scalar kernel."""
    B, H, W = shape
    x, mean = _frames(0, B, H, W)
    raw = torch.zeros(x.size + 4, device="cuda")
    gx = raw[1:1 + x.size]
    gx.copy_(torch.from_numpy(x).reshape(-1))
    assert gx.data_ptr() % 16 == 4
    _check_pack(hip_lib, x, gx, (torch.from_numpy(mean).cuda(),), R.RGB_MAX)


def test_pack_pair_past_the_grid_cap(hip_lib):
    """B * H * wpitch = 8192 * 256 + 2048 view pixels on the scalar kernel (one thread per view pixel, at most 8192 workgroups):
    the last 2048 pixels are a second trip of the grid-stride loop."""
    B, H, W = R.GRID_CAP_CASE
    assert R.GRID_CAP_THREADS < B * H * (W + 1)
    x, mean = _frames(0, B, H, W)
    _check_pack(hip_lib, x, torch.from_numpy(x).cuda(), (torch.from_numpy(mean).cuda(),), R.RGB_MAX, layouts=((0, 1),),
                dtypes=(torch.float16,))


# ---- (c) ft_flow_pack_pair_sums + ft_flow_mean_fold --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W4_SHAPES, ids=R.sid)
def test_pack_sums_and_mean_fold_are_exact(hip_lib, shape):
    """Chunk sums exact, mean bit-equal, inner pixels fp16(x / rgb_max), every padding pixel fp16(EXPECTED mean / rgb_max); pad 3 and
    1, the tight pitch and two wider; shift_n (1e-5 vs float64) with scale / shift present and NULL, Cout 64 and 7."""
    x, _ = _frames(0, *shape)
    _check_fold(hip_lib, x, R.RGB_MAX)


@pytest.mark.parametrize("shape", W4_SHAPES, ids=R.sid)
def test_pack_sums_impulses(hip_lib, shape):
    """One pixel per (sample, colour) at the first and last pixel of the first, a middle and the ragged last 4-row chunk."""
    _, H, W = shape
    for launch in R.impulse_launches(H, W, R.fold_impulse_positions(H, W)):
        _check_fold(hip_lib, R.impulse_pairs(len(launch) // 3, H, W, launch), R.RGB_MAX, configs=((3, 0),), what=f"impulses {launch}")


# ---- (d) ft_flow_mean_pack_pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=R.sid)
def test_fused_mean_pack_pair_is_exact(hip_lib, shape):
    """ONE state buffer per shape, zeroed once; fp16 and fp32; both views, the 6-channel view alone, the siamese view alone; five
    launches each on five frame sets that differ in every (sample, colour) sum, so a stale granule of the launch before — one
    among up to 126 — gives another mean.  After every launch: error word 0, mean and views bit-equal."""
    B, H, W = shape
    state = _fused_state(hip_lib, B, H, W)
    sets = [_frames(rep, B, H, W) for rep in range(R.FUSED_SETS)]
    gxs = [torch.from_numpy(x).cuda() for x, _ in sets]
    for dtype in (torch.float16, torch.float32):
        refs = [_fused_refs(x, R.RGB_MAX, dtype) for x, _ in sets]
        for use6, use3 in COMBOS:
            for rep in range(R.FUSED_SETS):
                _check_fused(hip_lib, gxs[rep], shape, sets[rep][1], refs[rep], R.RGB_MAX, dtype, state, use6, use3,
                             f"{R.sid(shape)} {dtype} views {use6, use3} frame set {rep}")


@pytest.mark.parametrize("shape", MULTI_WG_SHAPES, ids=R.sid)
def test_fused_impulses(hip_lib, shape):
    """One pixel per (sample, colour) at the first and last pixel of every workgroup's row share (2, 3, 5, 23, 42 workgroups)."""
    _, H, W = shape
    states = {}
    for launch in R.impulse_launches(H, W, R.fused_impulse_positions(H, W)):
        B = len(launch) // 3
        if B not in states:
            states[B] = _fused_state(hip_lib, B, H, W)
        v6, v3 = R.impulse_views(B, H, W, launch, FUSED_L6[0], W + FUSED_L6[1], FUSED_L3[0], W + FUSED_L3[1], np.float16)
        _check_fused(hip_lib, torch.from_numpy(R.impulse_pairs(B, H, W, launch)).cuda(), (B, H, W), R.impulse_mean(B, H, W),
                     (torch.from_numpy(v6).cuda(), torch.from_numpy(v3).cuda()), R.RGB_MAX, torch.float16, states[B], True, True,
                     f"{H}x{W} impulses {launch}")


def test_fused_epoch_wrap(hip_lib):
    """Every launch-count word (words [3 nW, 4 nW) of each sample's block) preset to 0xFFFFFFFE: three launches run epochs
    0xFFFFFFFF, 1 (0 is skipped: it is the tag of a zeroed state) and 2.  All exact, error word 0; the sweep is bounded, so a
    wrong wrap fails here and cannot hang."""
    B, H, W = SMALL
    nW = R.fused_plan(H, W)[1]
    state = _fused_state(hip_lib, B, H, W)
    blocks = state.t[:-1].view(B, 4 * nW)                     # per sample: 3 nW granules, then nW launch counts
    blocks[:, 3 * nW:] = 0xFFFFFFFE
    for rep, epoch in enumerate((0xFFFFFFFF, 1, 2)):
        x, mean = _frames(rep, B, H, W)
        _check_fused(hip_lib, torch.from_numpy(x).cuda(), SMALL, mean, _fused_refs(x, R.RGB_MAX, torch.float16), R.RGB_MAX, torch.float16,
                     state, True, True, f"epoch {epoch:#x}")
        assert bool((blocks[:, 3 * nW:] == epoch).all()), (epoch, blocks[:, 3 * nW:].cpu())
        assert bool((((blocks[:, :3 * nW] >> 32) & 0xFFFFFFFF) == epoch).all())


def test_refusals(hip_lib):
    """Shapes and arguments the entry points must refuse, by status (nothing here launches a kernel)."""
    words = hip_lib.ft_flow_mean_pack_pair_state_words
    buf = torch.zeros(4096, device="cuda")
    out = torch.zeros(4096, device="cuda")
    p, o, s = buf.data_ptr(), out.data_ptr(), _stream()
    assert p % 16 == 0

    def fused(B, H, W, ptr=p, rgb_max=255.0, y=o, y3=o, lpad=0, wpitch=None, dtype=FT_F16):
        wpitch = W if wpitch is None else wpitch
        return hip_lib.ft_flow_mean_pack_pair(ptr, rgb_max, y, lpad, wpitch, y3, lpad, wpitch, B, H, W, dtype, o, o, s)

    for (B, H, W) in ((1, 43, 6144), (2, 7, 9), (2, 8, 2)):
        assert int(words(B, H, W)) == 0 and fused(B, H, W) == FT_ERR_UNSUPPORTED, (B, H, W)
    assert int(words(2, 42, 6144)) == 2 * 4 * 42 + 1
    assert fused(1, 3, 4, ptr=p + 4) == FT_ERR_UNSUPPORTED
    assert int(words(512, 1, 4)) == 512 * 4 + 1 and int(words(513, 1, 4)) == 0 and fused(513, 1, 4) == FT_ERR_UNSUPPORTED
    assert int(words(12, 42, 6144)) == 12 * 4 * 42 + 1 and int(words(13, 42, 6144)) == 0
    assert fused(1, 3, 4, y=None, y3=None) == FT_ERR_INVALID_ARG
    assert fused(1, 3, 4, lpad=1, wpitch=4) == FT_ERR_INVALID_ARG
    assert fused(1, 3, 4, rgb_max=0.0) == FT_ERR_INVALID_ARG
    # the other entry points (ft_flow_rgb_mean takes no rgb_max)
    assert hip_lib.ft_flow_pack_pair_sums(p + 4, 255.0, o, 1, 3, 4, 1, 6, FT_F16, o, s) == FT_ERR_UNSUPPORTED
    assert hip_lib.ft_flow_pack_pair_sums(p, 0.0, o, 1, 3, 4, 1, 6, FT_F16, o, s) == FT_ERR_INVALID_ARG
    assert hip_lib.ft_flow_pack_pair(p, p, 0.0, o, 1, 3, 4, 0, 0, 4, FT_F16, s) == FT_ERR_INVALID_ARG
    assert hip_lib.ft_flow_mean_fold(p, 0.0, o, 1, 3, 4, 1, 6, FT_F16, p, None, None, 7, o, o, s) == FT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not buf.any() and not out.any()


# ---- rgb_max = 256 once per entry point that takes one ----------------------------------------------------------------------------
def test_rgb_max_256(hip_lib):
    B, H, W = SMALL
    x, mean = _frames(0, B, H, W)
    gx = torch.from_numpy(x).cuda()
    _check_pack(hip_lib, x, gx, (torch.from_numpy(mean).cuda(),), 256.0, layouts=((3, 6),))
    x9, mean9 = _frames(0, 2, 7, 9)
    _check_pack(hip_lib, x9, torch.from_numpy(x9).cuda(), (torch.from_numpy(mean9).cuda(),), 256.0, layouts=((3, 6),))
    _check_fold(hip_lib, x, 256.0, configs=((3, 2),))
    state = _fused_state(hip_lib, B, H, W)
    for dtype in (torch.float16, torch.float32):
        _check_fused(hip_lib, gx, SMALL, mean, _fused_refs(x, 256.0, dtype), 256.0, dtype, state, True, True, f"rgb_max 256 {dtype}")


# ---- (e) the three routes agree -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.ROUTE_SHAPES, ids=R.sid)
def test_three_routes_agree(hip_lib, shape):
    """fp16: ft_flow_pack_pair mode 0 (lpad 3, wpitch W + 6) == the fused kernel's 6-channel view, mode 1 == its siamese view, and
    all three routes return the same mean, bit for bit — kernel against kernel, no reference in between."""
    B, H, W = shape
    x, _ = _frames(0, B, H, W)
    gx = torch.from_numpy(x).cuda()
    _, mean_a = _run_mean(hip_lib, gx, B, H, W)
    y6, y3, mean_d = _fused_launch(hip_lib, gx, B, H, W, R.RGB_MAX, torch.float16, _fused_state(hip_lib, B, H, W))
    p6 = _run_pack(hip_lib, gx, mean_a, R.RGB_MAX, B, H, W, 0, FUSED_L6[0], W + FUSED_L6[1], torch.float16)
    p3 = _run_pack(hip_lib, gx, mean_a, R.RGB_MAX, B, H, W, 1, FUSED_L3[0], W + FUSED_L3[1], torch.float16)
    mean_c = _check_fold(hip_lib, x, R.RGB_MAX, configs=((3, 0),))
    assert _same_bits(mean_a, mean_d) and _same_bits(mean_a, mean_c)
    assert _same_bits(p6, y6) and _same_bits(p3, y3)


# ---- the comparisons are not vacuous: a reference flipped the way a broken kernel would be must NOT match -------------------------
def _wrong_sample(mean):
    return np.roll(mean.reshape(-1, 3), 1, axis=0).reshape(-1)


@pytest.mark.parametrize("entry", ["rgb_mean", "pack_pair", "pack_pair_sums", "mean_fold", "mean_pack_pair"])
def test_a_flipped_reference_differs(hip_lib, entry):
    """Per entry point: the reference of a frame with a dropped 4-pixel group / a dropped row, or built with another sample's mean,
    is unequal to what the kernel returns (which equals the unflipped reference by the tests above)."""
    B, H, W = SMALL
    x, mean = _frames(0, B, H, W)
    gx = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(1)
    dropped = [R.mutate(x, kind, rng)[0] for kind in ("drop_last_group", "drop_row")]
    bad_xn = R.normalise(x, _wrong_sample(mean))
    if entry == "rgb_mean":
        partial, got = _run_mean(hip_lib, gx, B, H, W)
        for xm in dropped:
            assert not _same_bits(got, R.expected_mean(xm)) and not _same_bits(partial, R.split_sums(xm))
        assert not _same_bits(got, _wrong_sample(mean))
    elif entry == "pack_pair":
        gm = torch.from_numpy(mean).cuda()
        for dtype in (torch.float16, torch.float32):
            got6 = _run_pack(hip_lib, gx, gm, R.RGB_MAX, B, H, W, 0, 3, W + 6, dtype)
            got3 = _run_pack(hip_lib, gx, gm, R.RGB_MAX, B, H, W, 1, 3, W + 6, dtype)
            assert not _same_bits(got6, R.view6(bad_xn, 3, W + 6, NP_OF[dtype]))
            assert not _same_bits(got3, R.view3(bad_xn, 3, W + 6, NP_OF[dtype]))
            for xm in dropped:
                assert not _same_bits(got6, R.view6(R.normalise(xm, mean), 3, W + 6, NP_OF[dtype]))
    elif entry in ("pack_pair_sums", "mean_fold"):
        pad, wpitch = 3, W + 6
        nchunk = R.fold_chunks(H)
        y = Guarded((B, H + 2 * pad, wpitch, 8), torch.float16, row_elems=wpitch * 8)
        partial = Guarded((B * 3, nchunk), torch.float32)
        check(hip_lib.ft_flow_pack_pair_sums(gx.data_ptr(), R.RGB_MAX, y.ptr(), B, H, W, pad, wpitch, FT_F16, partial.ptr(), _stream()))
        if entry == "pack_pair_sums":
            torch.cuda.synchronize()
            inner = y.t[:, pad:pad + H, pad:pad + W]
            assert _same_bits(inner, R.fold_view(x, mean, pad, wpitch)[:, pad:pad + H, pad:pad + W])
            for xm in dropped:
                assert not _same_bits(partial.t, R.chunk_sums(xm))
                assert not _same_bits(inner, R.fold_view(xm, mean, pad, wpitch)[:, pad:pad + H, pad:pad + W])
        else:
            shn, got = Guarded((B, 7), torch.float32), Guarded((B * 3,), torch.float32)
            wsum = torch.ones((7, 8), device="cuda")
            check(hip_lib.ft_flow_mean_fold(partial.ptr(), R.RGB_MAX, y.ptr(), B, H, W, pad, wpitch, FT_F16, wsum.data_ptr(), None, None, 7,
                                            shn.ptr(), got.ptr(), _stream()))
            torch.cuda.synchronize()
            assert _same_bits(y.t, R.fold_view(x, mean, pad, wpitch))
            assert not _same_bits(y.t, R.fold_view(x, _wrong_sample(mean), pad, wpitch))
            for xm in dropped:
                assert not _same_bits(got.t, R.expected_mean(xm))
            assert np.abs(shn.t.cpu().numpy() - R.fold_shift(_wrong_sample(mean), np.ones((7, 8)), None, None)).max() > 1e-5
    else:
        y6, y3, got = _fused_launch(hip_lib, gx, B, H, W, R.RGB_MAX, torch.float16, _fused_state(hip_lib, B, H, W))
        assert not _same_bits(y6, R.view6(bad_xn, FUSED_L6[0], W + FUSED_L6[1], np.float16))
        assert not _same_bits(y3, R.view3(bad_xn, FUSED_L3[0], W + FUSED_L3[1], np.float16))
        for xm in dropped:
            assert not _same_bits(got, R.expected_mean(xm))
            assert not _same_bits(y6, R.view6(R.normalise(x, R.expected_mean(xm)), FUSED_L6[0], W + FUSED_L6[1], np.float16))
