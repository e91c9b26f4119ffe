"""Shapes, N(0, 1) inputs, float64 references and derived bounds shared by test_conv_direct_bound_cpu.py / test_conv_direct_bound_gpu.py:
one case per form of ft_conv_direct_fwd (the transposed form has deconv_direct_cases.py), plus plain and deliberately degraded fp32
evaluations in numpy for the CPU test.

x, w and the residual are N(0, 1) draws rounded to fp16; BatchNorm has mixed-sign gammas (deconv_direct_cases.bn_of).  Eight output
channels of every case keep ONE weight only (their other draws are zeroed): an output element of such a channel is a single product,
its S is small and the bound there is little more than the one rounding to fp16 — the elements where a precision-class mistake shows
even under the worst-case accumulation term of a long K."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import synth

import exact_cases as ec
from conv_bound import derived_bound
from deconv_direct_cases import bn_of

SEED = 53
SLOPE = float(np.float32(0.1))          # the LeakyReLU slope as the fp32 the descriptor carries

# the cases of part 1 (exact_cases.py) whose shapes are used again, one per form; "shortcut.stride1" is the K-concatenated GEMM
NAMES = ["ragged_pixels", "ragged_pixels_wide", "stationary_ragged", "shortcut.stride1", "tiny_3x5", "c1024_tiny", "leaky_256_512_s2_slice",
         "s2_whole_odd_map", "s2_pair_odd_batch", "s2_strips_ragged", "strips_ragged_last", "ragged_patches"]


def case_of(name):
    return next(c for c in ec.DIRECT_CONVS if c["name"] == name)


def single_weight_channels(cout):
    return [1, 2, 3, 4, cout - 5, cout - 4, cout - 2, cout - 1]


def _single_weight_channels(w, cout):
    """Eight channels keep one weight each: the last tap of the last input channel, the first tap of the first, and six in between."""
    w = w.clone()
    _, cin, k, _ = w.shape
    where = ((cin - 1, k - 1, k - 1), (0, 0, 0), (cin // 2, k // 2, 0), (cin // 3, 0, k - 1), (63, k - 1, 0), (64, k // 2, k // 2), (cin - 65, 0, k // 2),
             (cin // 2 + 1, k - 1, k // 2))
    for co, (ci, ky, kx) in zip(single_weight_channels(cout), where):
        ci %= cin
        keep = w[co, ci, ky, kx].clone()
        w[co] = 0.0
        w[co, ci, ky, kx] = keep if keep != 0 else 1.0
    return w


def _fold(bn, bias, cout):
    """(scale, shift) as the fp32 tables hold them, in float64 (hip_ops.fold_scale_shift restated)."""
    if bn is None:
        return torch.ones(cout, dtype=torch.float64), (bias.float().double() if bias is not None else torch.zeros(cout, dtype=torch.float64))
    s64 = bn["weight"].double() / torch.sqrt(bn["running_var"].double() + bn["eps"])
    sh64 = bn["bias"].double() - bn["running_mean"].double() * s64
    if bias is not None:
        sh64 = sh64 + bias.double() * s64
    return s64.float().double(), sh64.float().double()


def _act(v, act):
    if act == "relu":
        return torch.clamp(v, min=0.0)
    if act == "leaky":
        return torch.where(v > 0, v, v * SLOPE)
    return v


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs (fp16-representable, fp32), and in float64: scale / shift, the bare sum `pre`, S = sum |x * w| per output element, `want`
    and the bound.  The shortcut form folds its two BN scales into fp16 weights: its reference takes fp16(fp32(w) * fp32(scale)) as
    the weights and a scale of 1."""
    if name.startswith("shortcut."):
        _, N, Hx, Wx, planes, cin_x, s = next(c for c in ec.DIRECT_SHORTCUT if c[0] == name.split(".", 1)[1])
        cout = 4 * planes
        H, W = (Hx - 1) // s + 1, (Wx - 1) // s + 1
        w3 = _single_weight_channels(synth.normal(SEED, name + ".w3", (cout, planes, 1, 1)).half().float(), cout)
        wd = synth.normal(SEED, name + ".wd", (cout, cin_x, 1, 1)).half().float()
        wd[single_weight_channels(cout)] = 0.0
        bn3, bnd = bn_of(name + ".bn3", cout, SEED), bn_of(name + ".bnd", cout, SEED)
        t2 = synth.normal(SEED, name + ".t2", (N, planes, H, W)).half().float()
        x = synth.normal(SEED, name + ".x", (N, cin_x, Hx, Wx)).half().float()
        (s3, sh3), (sd, shd) = _fold(bn3, None, cout), _fold(bnd, None, cout)
        w3f = (w3 * s3.float().view(-1, 1, 1, 1)).half().double()           # fp16(fp32(w) * fp32(scale))
        wdf = (wd * sd.float().view(-1, 1, 1, 1)).half().double()
        shift = (sh3.float() + shd.float()).double()                        # the two fp32 shifts, added in fp32
        pre = ec.conv64(t2.double(), w3f) + ec.conv64(x.double(), wdf, s)
        S = ec.conv64(t2.double().abs(), w3f.abs()) + ec.conv64(x.double().abs(), wdf.abs(), s)
        want = torch.clamp(pre + shift.view(1, -1, 1, 1), min=0.0)
        one = torch.ones(cout, dtype=torch.float64)
        return {"kind": "shortcut", "t2": t2, "x": x, "w3": w3, "wd": wd, "bn3": bn3, "bnd": bnd, "stride": s, "w3f": w3f, "wdf": wdf,
                "scale": one, "shift": shift, "pre": pre, "S": S, "want": want, "act": "relu", "res": None, "K": planes + cin_x,
                "bound": derived_bound(planes + cin_x, S, pre, one, want)}
    c = case_of(name)
    N, Cin, H, W, Cout, k, s, p = (c[f] for f in ("N", "Cin", "H", "W", "Cout", "k", "s", "p"))
    w = _single_weight_channels(synth.normal(SEED, name + ".w", (Cout, Cin, k, k)).half().float(), Cout)
    x = synth.normal(SEED, name + ".x", (N, Cin, H, W)).half().float()
    bn = bn_of(name + ".bn", Cout, SEED) if "bn" in c["norm"] else None
    bias = synth.normal(SEED, name + ".bias", (Cout,), 0.2) if "bias" in c["norm"] else None
    scale, shift = _fold(bn, bias, Cout)
    pre = ec.conv64(x.double(), w.double(), s, p)
    S = ec.conv64(x.double().abs(), w.double().abs(), s, p)
    v = pre * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res, extra = None, []
    if c["res"]:
        res = synth.normal(SEED, name + ".r", tuple(pre.shape)).half().float()
        v = v + res.double()
        extra.append(v)                     # the residual add
    want = _act(v, c["act"])
    if c["act"] == "leaky":
        extra.append(want)                  # the leaky multiply
    K = k * k * Cin
    return {"kind": "conv", "case": c, "x": x, "w": w, "bn": bn, "bias": bias, "res": res, "scale": scale, "shift": shift, "pre": pre, "S": S,
            "want": want, "act": c["act"], "K": K, "bound": derived_bound(K, S, pre, scale, want, extra)}


# ---- plain and degraded fp32 evaluations (numpy) ---------------------------------------------------------------------------------------
def _columns(x, k, stride, pad):
    """im2col in tap-major order: [M, k * k * Cin] with column (ky * k + kx) * Cin + ci, fp32."""
    N, Cin = x.shape[:2]
    cols = F.unfold(x, k, padding=pad, stride=stride)                                # [N, Cin * k * k, L], ci-major
    L = cols.shape[2]
    return cols.view(N, Cin, k * k, L).permute(0, 3, 2, 1).reshape(N * L, k * k * Cin).contiguous().numpy()


def channel_subset(cout, n=12):
    """The single-weight channels and a spread of dense ones: what the numpy evaluations compute."""
    pick = sorted(set(single_weight_channels(cout) + [int(i) for i in np.linspace(0, cout - 1, n)]))
    return pick


def operands(r, chans):
    """(A [M, K] fp32, Wm [K, len(chans)] fp32) of a case: out[m, c] = sum_k A[m, k] Wm[k, c], K tap-major, so that 64 consecutive k
    are 64 input channels of one tap (the shortcut form: the channels of t2, then those of x)."""
    if r["kind"] == "shortcut":
        A = np.concatenate([_columns(r["t2"], 1, 1, 0), _columns(r["x"], 1, r["stride"], 0)], axis=1)
        Wm = torch.cat([r["w3f"][chans, :, 0, 0], r["wdf"][chans, :, 0, 0]], dim=1).t().float().contiguous().numpy()
        return A, Wm
    c = r["case"]
    A = _columns(r["x"], c["k"], c["s"], c["p"])
    Wm = r["w"][chans].permute(2, 3, 1, 0).reshape(-1, len(chans)).contiguous().numpy()          # (ky, kx, ci) rows
    return A, Wm


def truncate_to_fp16(v):
    """fp32 -> fp16 with the discarded bits dropped (round toward zero)."""
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h)


def rows_of(t, chans, rows):
    """[N, C, H, W] -> the [pixels, len(chans)] matrix the numpy evaluations work on, restricted to `rows`."""
    m = t[:, chans].permute(0, 2, 3, 1).reshape(-1, len(chans))
    return m if rows is None else m[rows]


def evaluate(r, chans, mode="plain", max_rows=8192):
    """The layer on the channels `chans` in fp32, one accumulator per output element, K ascending (taps, then channels), then fp32
    scale / shift (+ residual, activation) and one rounding to fp16.  mode: plain; scale16 = the scale table (the shift table of the
    shortcut form, which has no scale table) rounded to fp16; chunk16 = each 64-channel partial sum rounded to fp16 before it is added;
    truncate = the final rounding replaced by truncation.  Maps of more than max_rows pixels: the first and the last max_rows / 2.
    Returns (float64 [pixels, len(chans)], rows or None = all)."""
    A, Wm = operands(r, chans)
    rows = None
    if A.shape[0] > max_rows:
        rows = np.concatenate([np.arange(max_rows // 2), np.arange(A.shape[0] - max_rows // 2, A.shape[0])])
        A = np.ascontiguousarray(A[rows])
    M, K = A.shape
    acc = np.zeros((M, len(chans)), dtype=np.float32)
    if mode == "chunk16":
        for k0 in range(0, K, 64):
            part = np.zeros_like(acc)
            for k in range(k0, min(k0 + 64, K)):
                part += A[:, k, None] * Wm[k]
            acc += part.astype(np.float16).astype(np.float32)
    else:
        for k in range(K):
            acc += A[:, k, None] * Wm[k]             # exact products, one fp32 rounding per add
    scale, shift = r["scale"][chans].numpy().astype(np.float32), r["shift"][chans].numpy().astype(np.float32)
    if mode == "scale16":
        if r["kind"] == "shortcut":
            shift = shift.astype(np.float16).astype(np.float32)
        else:
            scale = scale.astype(np.float16).astype(np.float32)
    v = acc * scale + shift
    if r["res"] is not None:
        v = v + rows_of(r["res"], chans, rows).numpy()
    if r["act"] == "relu":
        v = np.maximum(v, np.float32(0))
    elif r["act"] == "leaky":
        v = np.where(v > 0, v, v * np.float32(SLOPE))
    h = truncate_to_fp16(v) if mode == "truncate" else v.astype(np.float16)
    return torch.from_numpy(h.astype(np.float64)), rows


# ---- impulse cases: one per tap geometry, compared exactly ----------------------------------------------------------------------------
# name, N, Cin, H, W, Cout, k, stride, pad, the form ft_conv_direct_stream_id must report
IMPULSES = [("impulse_3x3_s1", 3, 512, 6, 5, 512, 3, 1, 1, "c3"), ("impulse_3x3_s2_whole", 3, 512, 13, 9, 512, 3, 2, 1, "c3s2"),
            ("impulse_3x3_s2_paired", 51, 512, 12, 16, 512, 3, 2, 1, "c3s2_pair"), ("impulse_3x3_s2_strips", 9, 512, 26, 20, 512, 3, 2, 1, "c3s2"),
            ("impulse_5x5_s2", 3, 64, 21, 17, 128, 5, 2, 2, "ws5")]
IMPULSE_SHORTCUT = ("impulse_shortcut_s2", 3, 9, 7, 256, 512, 2)          # name, N, Hx, Wx, planes, Cin of x, stride


def impulse_input(N, C, H, W):
    """1 at the first corner of the first image (channel 3), 2 at the last corner of the last image (last channel)."""
    x = torch.zeros((N, C, H, W))
    x[0, 3, 0, 0] = 1.0
    x[N - 1, C - 1, H - 1, W - 1] = 2.0
    return x
