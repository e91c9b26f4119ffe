"""Shapes, inputs, float64 reference and the derived error bound shared by test_deconv_direct_cpu.py / test_deconv_direct_gpu.py
(the transposed form of ft_conv_direct_fwd: ConvTranspose2d(4, 2, 1) on whole small maps as one GEMM + col2im)."""
import functools

import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import synth

from conv_bound import derived_bound

# name, N, Hi, Wi, Cin, Cout, (x_coff, y_coff) of the views inside wider buffers
CASES = [
    ("n1_8x6_k2048_unrolled", 1, 8, 6, 2048, 48, (0, 0)),      # Cin 2048: the unrolled 32-chunk walk; one image in a two-image tile
    ("n3_8x6_ragged_last_tile", 3, 8, 6, 256, 16, (0, 0)),     # second tile holds one image; Cin 256: the unrolled 4-chunk walk
    ("n5_6x8", 5, 6, 8, 320, 48, (0, 0)),                      # Cin 320: the run-time loop, 5 chunks (not a multiple of the ring)
    ("n9_4x3_ipw8", 9, 4, 3, 256, 256, (0, 0)),                # eight images per tile, 16 channel blocks, ragged second tile
    ("n2_9x10_idle_rows", 2, 9, 10, 320, 16, (0, 0)),          # 90 pixels: one image per tile, six idle rows
    ("n3_8x6_views", 3, 8, 6, 256, 48, (32, 64)),              # x / y views inside wider buffers
]
IDS = [c[0] for c in CASES]


def bn_of(name, c, seed=41):
    return {"weight": synth.uniform(seed, name + "g", (c,), 0.5, 1.5) * torch.where(torch.arange(c) % 3 == 0, -1.0, 1.0),
            "bias": synth.normal(seed, name + "b", (c,), 0.1), "running_mean": synth.normal(seed, name + "m", (c,), 0.1),
            "running_var": synth.uniform(seed, name + "v", (c,), 0.5, 1.5), "eps": 1e-5}


@functools.lru_cache(maxsize=None)
def reference(name):
    """x, w (fp16-representable, fp32), bn, and in float64: the folded scale / shift, the bare sum `pre`, S = sum |x * w| per
    output element, the result `want` = relu(pre * scale + shift) and the bound below."""
    _, N, Hi, Wi, Cin, Cout, _ = next(c for c in CASES if c[0] == name)
    seed = 41
    x = synth.normal(seed, name + ".x", (N, Cin, Hi, Wi)).half().float()
    w = synth.normal(seed, name + ".w", (Cin, Cout, 4, 4)).half().float()          # N(0, 1), rounded to fp16
    bn = bn_of(name, Cout)
    s64 = bn["weight"].double() / torch.sqrt(bn["running_var"].double() + bn["eps"])        # hip_ops.fold_scale_shift
    scale, shift = s64.float().double(), (bn["bias"].double() - bn["running_mean"].double() * s64).float().double()   # as the fp32 tables hold them
    pre = F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1)
    S = F.conv_transpose2d(x.double().abs(), w.double().abs(), stride=2, padding=1)
    want = F.relu(pre * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    return {"x": x, "w": w, "bn": bn, "scale": scale, "shift": shift, "pre": pre, "S": S, "want": want,
            "bound": bound(Cin, S, pre, scale, want)}


def bound(Cin, S, pre, scale, want):
    """Per element: worst-case fp32 accumulation of the 4 * Cin exact fp16 x fp16 products of an output element (every partial sum
    is at most S, one rounding of 2^-24 relative each), doubled for the summation order inside an MFMA; the rounding of the sum
    into the scale / shift FMA; one rounding to fp16 (2^-11 relative, 2^-25 absolute in the subnormal range)."""
    return derived_bound(4 * Cin, S, pre, scale, want)


def sequential_fp32(x, w, scale, shift):
    """The same layer with every product added into ONE fp32 accumulator per output element, taps ascending, channels ascending
    inside a tap, then fp32 scale / shift, relu and a rounding to fp16 — plain numpy, no fused operation."""
    import numpy as np
    xn, wn = x.numpy().astype(np.float32), w.numpy().astype(np.float32)
    N, Cin, Hi, Wi = xn.shape
    Cout = wn.shape[1]
    acc = np.zeros((N, 2 * Hi, 2 * Wi, Cout), dtype=np.float32)
    for ky in range(4):
        iy = [i for i in range(Hi) if 0 <= 2 * i - 1 + ky < 2 * Hi]
        for kx in range(4):
            ix = [i for i in range(Wi) if 0 <= 2 * i - 1 + kx < 2 * Wi]
            oy, ox = slice(2 * iy[0] - 1 + ky, 2 * iy[-1] + ky, 2), slice(2 * ix[0] - 1 + kx, 2 * ix[-1] + kx, 2)
            xs = xn[:, :, iy[0]:iy[-1] + 1, ix[0]:ix[-1] + 1]
            for ci in range(Cin):
                acc[:, oy, ox, :] += xs[:, ci, :, :, None] * wn[ci, :, ky, kx]      # exact products, one fp32 rounding per add
    out = acc * scale.numpy().astype(np.float32) + shift.numpy().astype(np.float32)
    out = np.maximum(out, np.float32(0)).astype(np.float16)
    return torch.from_numpy(out.astype(np.float64)).permute(0, 3, 1, 2).contiguous()
