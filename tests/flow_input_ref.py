"""Reference and inputs for the exact tests of the flow input kernels (csrc/aux_ops.hip: ft_flow_rgb_mean, ft_flow_pack_pair,
ft_flow_pack_pair_sums + ft_flow_mean_fold, ft_flow_mean_pack_pair).  numpy only.

Why exact: the frames hold INTEGERS and a colour's sum over both frames stays below 2^22, so every partial sum a kernel forms,
in whatever order, is an exact fp32 integer.  The mean is then ONE rounded product, fp32(S) * fp32(1 / (2 H W)), and a packed
value is one correctly rounded subtract, one correctly rounded divide (the build passes no fast-math flag) and one
round-to-nearest-even cast: predictable bit for bit, no tolerance.  Adjacent sums S and S + 1 give different fp32 means at every
shape used (tests/test_flow_input_cpu.py checks that), so one dropped or doubled pixel shows.

Layout of the network input: inputs[b, c, f, y, x] (colour before frame); the mean is over both frames of a colour."""
import numpy as np

F32 = np.float32
RGB_MAX = 255.0
SPLITS = 64                                 # FT_RGB_MEAN_SPLITS
FOLD_ROWS = 4                               # FT_PACK_SUMS_ROWS
FUSED_ITEMS = 6 * 256                       # 4-pixel groups a workgroup of the fused kernel holds per plane (kMpNit * 256)
FUSED_MAX_GRID = 512                        # kMpMaxGrid
SUM_LIMIT = 2 ** 22

# (B, H, W): the smallest shapes at which each path of the five entry points can still go wrong
SHAPES = [
    (2, 1, 4), (3, 3, 4),                   # L < 64 splits: most splits empty; one 4-pixel group per row; fused: one workgroup
    (2, 7, 9),                              # odd W: scalar mean path, scalar pack kernel; the fused and fold forms refuse
    (3, 5, 26),                             # L % 4 == 0 but the per-split length is not: scalar mean path
    (2, 9, 40), (3, 11, 8),                 # vector / scalar mean path with trailing empty splits; fold: ragged last chunk
    (2, 13, 512),                           # fused: 2 workgroups, rows 7 + 6
    (3, 25, 512),                           # fused: 3 workgroups, rows 9 + 9 + 7
    (2, 7, 2048),                           # fused: 3 workgroups, rows 3 + 3 + 1
    (2, 5, 6144),                           # fused: 5 workgroups of one row, every lane holds all six groups
    (3, 130, 100), (2, 50, 260),            # ragged: rows 44 + 44 + 42 and 17 + 17 + 16
    (3, 160, 832),                          # mean: one round of the unrolled loop + a 16-lane tail; fused: 23 workgroups
    (2, 42, 6144),                          # fused: 42 workgroups per sample (the most); mean: second unrolled round partial
]
# one batch past the 8192-block grid cap of the pack kernels (scalar kernel: one thread per view pixel, B * H * wpitch of them)
GRID_CAP_THREADS = 8192 * 256
GRID_CAP_CASE = (2, 1025, 1023)             # with wpitch 1024: 2 * 1025 * 1024 = cap + 2048 view pixels
FUSED_SETS = 5                              # frame sets per state buffer in the fused kernel's test
ROUTE_SHAPES = [(3, 25, 512), (3, 160, 832)]


def sid(shape):
    return "x".join(str(v) for v in shape)


def vmax(H, W):
    return min(255, (SUM_LIMIT - 1) // (2 * H * W))


def colour_sums(x):
    """Exact integer sum per (sample, colour) over both frames: int64 [B, 3]."""
    B = x.shape[0]
    return x.astype(np.int64).reshape(B, 3, -1).sum(-1)


def int_pairs(seed, B, H, W):
    """[B,3,2,H,W] float32 of integers in [1, vmax]; slot k = b * 3 + c draws from [1, hi_k] with hi_k rising with k, and a
    last pass moves single pixels by one until the 3B sums are pairwise different (so are the means then)."""
    vm = vmax(H, W)
    assert vm >= 2, (H, W)
    rng = np.random.default_rng(seed)
    n = 3 * B
    x = np.empty((n, 2 * H * W), dtype=np.int64)
    for k in range(n):
        hi = max(2, vm - ((n - 1 - k) * (vm - 2)) // n)
        x[k] = rng.integers(1, hi + 1, size=2 * H * W)
    seen = set()
    for k in range(n):
        i = 0
        while int(x[k].sum()) in seen:
            if x[k, i] < vm:
                x[k, i] += 1
            else:
                i += 1
        seen.add(int(x[k].sum()))
    return x.reshape(B, 3, 2, H, W).astype(F32)


def impulse_pairs(B, H, W, positions):
    """Zero except one pixel of value vmax per (sample, colour): positions[b * 3 + c] = (frame, y, x)."""
    assert len(positions) == 3 * B
    x = np.zeros((B, 3, 2, H, W), dtype=F32)
    for k, (f, y, xx) in enumerate(positions):
        x[k // 3, k % 3, f, y, xx] = vmax(H, W)
    return x


def impulse_mean(B, H, W):
    """Expected mean of any impulse_pairs batch: every colour sum is vmax."""
    return mean_of_sums(np.full(3 * B, vmax(H, W)), H, W)


def impulse_views(B, H, W, positions, lpad6, wpitch6, lpad3, wpitch3, dtype, rgb_max=RGB_MAX):
    """view6 and view3 of normalise(impulse_pairs(...)) without forming the frames: a constant per (sample, colour) for the zero
    pixels, one other value at the impulse (tests/test_flow_input_cpu.py holds it to the general path)."""
    m = impulse_mean(B, H, W)
    bg = ((F32(0) - m) / F32(rgb_max)).astype(dtype).reshape(B, 3)
    pk = ((F32(vmax(H, W)) - m) / F32(rgb_max)).astype(dtype).reshape(B, 3)
    v6 = np.zeros((B, H, wpitch6, 8), dtype=dtype)
    v3 = np.zeros((2 * B, H, wpitch3, 4), dtype=dtype)
    for f in range(2):
        v6[:, :, lpad6:lpad6 + W, 3 * f:3 * f + 3] = bg[:, None, None, :]
        v3[f * B:(f + 1) * B, :, lpad3:lpad3 + W, :3] = bg[:, None, None, :]
    for k, (f, y, xx) in enumerate(positions):
        b, c = divmod(k, 3)
        v6[b, y, lpad6 + xx, 3 * f + c] = pk[b, c]
        v3[f * B + b, y, lpad3 + xx, c] = pk[b, c]
    return v6, v3


def mean_of_sums(S, H, W):
    """fp32(S) * (1 / fp32(2 H W)): the one rounded product every kernel forms."""
    return (np.asarray(S).astype(F32) * (F32(1) / F32(2 * H * W))).astype(F32)


def expected_mean(x):
    _, _, _, H, W = x.shape
    return mean_of_sums(colour_sums(x), H, W).reshape(-1)


def normalise(x, mean, rgb_max=RGB_MAX):
    """(x - mean) / rgb_max, every step in float32: [B,3,2,H,W]."""
    B = x.shape[0]
    m = np.asarray(mean, dtype=F32).reshape(B, 3, 1, 1, 1)
    out = (x.astype(F32) - m) / F32(rgb_max)
    assert out.dtype == F32
    return out


def view6(xn, lpad, wpitch, dtype):
    """The 6-channel view [B,H,wpitch,8]: frame 0's colours, frame 1's, two zeros; zero pad columns."""
    B, _, _, H, W = xn.shape
    v = np.zeros((B, H, wpitch, 8), dtype=dtype)
    for f in range(2):
        v[:, :, lpad:lpad + W, 3 * f:3 * f + 3] = xn[:, :, f].transpose(0, 2, 3, 1).astype(dtype)
    return v


def view3(xn, lpad, wpitch, dtype):
    """The siamese view [2B,H,wpitch,4]: image f * B + b, channels (r, g, b, 0); zero pad columns."""
    B, _, _, H, W = xn.shape
    v = np.zeros((2 * B, H, wpitch, 4), dtype=dtype)
    for f in range(2):
        v[f * B:(f + 1) * B, :, lpad:lpad + W, :3] = xn[:, :, f].transpose(0, 2, 3, 1).astype(dtype)
    return v


def fold_view(x, mean, pad, wpitch, rgb_max=RGB_MAX):
    """The fold's row-and-column padded view fp16 [B,H+2pad,wpitch,8]: fp16(x / rgb_max) inside, fp16(mean / rgb_max) in every
    padding pixel (channels 6, 7 zero everywhere)."""
    B, _, _, H, W = x.shape
    m16 = (np.asarray(mean, dtype=F32).reshape(B, 3) / F32(rgb_max)).astype(np.float16)
    v = np.zeros((B, H + 2 * pad, wpitch, 8), dtype=np.float16)
    v[..., 0:3] = m16[:, None, None, :]
    v[..., 3:6] = m16[:, None, None, :]
    xs = (x.astype(F32) / F32(rgb_max)).astype(np.float16)
    for f in range(2):
        v[:, pad:pad + H, pad:pad + W, 3 * f:3 * f + 3] = xs[:, :, f].transpose(0, 2, 3, 1)
    return v


def fold_shift(mean, wsum, scale, shift, rgb_max=RGB_MAX):
    """shift_n[b][co] = shift[co] - scale[co] * sum_c m16[c % 3] * wsum[co][c] in float64 (scale None = 1, shift None = 0)."""
    B = np.asarray(mean).size // 3
    m16 = (np.asarray(mean, dtype=F32).reshape(B, 3) / F32(rgb_max)).astype(np.float16).astype(np.float64)
    w = np.asarray(wsum, dtype=np.float64)
    corr = m16 @ w[:, 0:3].T + m16 @ w[:, 3:6].T
    sc = 1.0 if scale is None else np.asarray(scale, dtype=np.float64)[None]
    sh = 0.0 if shift is None else np.asarray(shift, dtype=np.float64)[None]
    return sh - sc * corr


# ---- the work split of each kernel, restated as plain arithmetic (for placing inputs and for the exact partial sums) ----------
def split_spans(H, W):
    """ft_flow_rgb_mean: span [lo, hi) of each of the 64 splits in a colour's 2 H W floats (hi <= lo: empty)."""
    L = 2 * H * W
    per = (L + SPLITS - 1) // SPLITS
    return per, [(s * per, min(L, s * per + per)) for s in range(SPLITS)]


def split_sums(x):
    """Exact partial[bc * 64 + split]: float32 [B*3, 64]."""
    B, _, _, H, W = x.shape
    flat = x.astype(np.int64).reshape(B * 3, -1)
    _, spans = split_spans(H, W)
    return np.stack([flat[:, lo:hi].sum(-1) if hi > lo else np.zeros(B * 3, np.int64) for lo, hi in spans], 1).astype(F32)


def mean_path_is_vector(H, W):
    L = 2 * H * W
    per, _ = split_spans(H, W)
    return L % 4 == 0 and per % 4 == 0


def fold_chunks(H):
    return (H + FOLD_ROWS - 1) // FOLD_ROWS


def chunk_sums(x):
    """Exact partial[(b*3+c) * nchunk + chunk] of ft_flow_pack_pair_sums: float32 [B*3, nchunk]."""
    B, _, _, H, W = x.shape
    xi = x.astype(np.int64).reshape(B * 3, 2, H, W)
    return np.stack([xi[:, :, r:r + FOLD_ROWS].sum((1, 2, 3)) for r in range(0, H, FOLD_ROWS)], 1).astype(F32)


def fused_plan(H, W):
    """(rows per workgroup R, workgroups per sample n) of ft_flow_mean_pack_pair, or None where its planner refuses."""
    if H <= 0 or W < 4 or W % 4:
        return None
    r = (FUSED_ITEMS * 4) // W
    if r < 1:
        return None
    r = min(r, H)
    n = -(-H // r)
    if 3 * n > 128:
        return None
    return -(-H // n), n


def fused_row_shares(H, W):
    R, n = fused_plan(H, W)
    return [min(R, H - w * R) for w in range(n)]


def fused_state_words(B, H, W):
    p = fused_plan(H, W)
    if B <= 0 or p is None or B * p[1] > FUSED_MAX_GRID:
        return 0
    return B * 4 * p[1] + 1


# ---- impulse positions (frame, y, x) ---------------------------------------------------------------------------------------
def flat_position(p, H, W):
    """Element p of a colour's 2 H W floats (frame-major) as (frame, y, x)."""
    return (p // (H * W), (p % (H * W)) // W, p % W)


def mean_impulse_positions(H, W):
    """ft_flow_rgb_mean: first and last pixel of each frame; first and last element of splits 0, 1, 31, 63 (where not empty);
    at 160 x 832 the last element before and the first of the tail loop (float4 1023 / 1024 of split 0)."""
    L, HW = 2 * H * W, H * W
    flat = [0, HW - 1, HW, L - 1]
    _, spans = split_spans(H, W)
    for s in (0, 1, 31, 63):
        lo, hi = spans[s]
        if hi > lo:
            flat += [lo, hi - 1]
    if (H, W) == (160, 832):
        flat += [4 * 1024 - 1, 4 * 1024]
    return [flat_position(p, H, W) for p in dict.fromkeys(flat)]


def fold_impulse_positions(H, W):
    """ft_flow_pack_pair_sums: first and last pixel of the first, a middle and the (ragged) last 4-row chunk."""
    n = fold_chunks(H)
    pos = []
    for i, ch in enumerate(dict.fromkeys((0, n // 2, n - 1))):
        r0, r1 = ch * FOLD_ROWS, min(H, ch * FOLD_ROWS + FOLD_ROWS) - 1
        pos += [(i % 2, r0, 0), ((i + 1) % 2, r1, W - 1)]
    return pos


def fused_impulse_positions(H, W):
    """ft_flow_mean_pack_pair: first and last pixel of every workgroup's row share."""
    R, n = fused_plan(H, W)
    pos = []
    for w, rows in enumerate(fused_row_shares(H, W)):
        pos += [(w % 2, w * R, 0), ((w + 1) % 2, w * R + rows - 1, W - 1)]
    return pos


def impulse_batch(H, W):
    """Samples per impulse launch: up to 16, fewer where the frames would pass about 12 MB."""
    return int(max(2, min(16, (12 * 2 ** 20 + 2 ** 19) // (24 * H * W))))


def impulse_launches(H, W, positions):
    """Split `positions` into launches of 3 B positions each (the last one padded by repeating its first entries)."""
    per = 3 * impulse_batch(H, W)
    out = []
    for i in range(0, len(positions), per):
        chunk, j = list(positions[i:i + per]), 0
        while len(chunk) % 3:
            chunk.append(chunk[j])
            j += 1
        out.append(chunk)
    return out


# ---- mutations of the data a wrong reduction would amount to (each must move the expected mean) ---------------------------------
def mutate(x, kind, rng):
    """A copy of x with one (sample, colour) slot changed as a broken kernel would see it; returns (copy, slot)."""
    B, _, _, H, W = x.shape
    y = x.copy()
    k = int(rng.integers(3 * B))
    b, c = divmod(k, 3)
    f, r, col = int(rng.integers(2)), int(rng.integers(H)), int(rng.integers(W))
    if kind == "drop_pixel":
        y[b, c, f, r, col] = 0
    elif kind == "double_pixel":
        y[b, c, f, r, col] *= 2
    elif kind == "drop_row":
        y[b, c, f, r, :] = 0
    elif kind == "drop_last_group":
        y[b, c, f, r, max(0, W - 4):] = 0
    elif kind == "drop_split":
        _, spans = split_spans(H, W)
        live = [s for s in spans if s[1] > s[0]]
        lo, hi = live[int(rng.integers(len(live)))]
        y[b, c].reshape(-1)[lo:hi] = 0
    else:
        raise ValueError(kind)
    return y, k


MUTATIONS = ("drop_pixel", "double_pixel", "drop_row", "drop_last_group", "drop_split")
