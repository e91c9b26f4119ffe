"""The case table of the in-network correlation (ft_correlation_nhwc_fwd), shared by test_correlation_forms_cpu.py (which kernel
form each row reaches, the reference, the bound) and test_correlation_forms_gpu.py (the kernels themselves).  Every row is the
smallest shape that reaches one edge of one of the four kernels behind the entry point; nothing here needs more than a few MB."""
import collections

import torch

from correlation_ref import correlation_nhwc_ref
from flowtrack.pytorch_amd import synth

VALU, MFMA, ROWS, ROWS64 = 0, 1, 2, 3          # FT_CORR_FORM_*
FORM_NAMES = {VALU: "valu", MFMA: "mfma", ROWS: "rows", ROWS64: "rows64"}
F16, F32 = 0, 1                                # FT_F16 / FT_F32
NONE, RELU, LEAKY = 0, 1, 2                    # FT_ACT_*
INVALID_ARG, UNSUPPORTED = 1, 2                # FT_ERR_*
SENTINEL = -77.0                               # exact in fp16; 1/C sum a b of N(0, 1) features never gets near it

# `form` is what ft_correlation_nhwc_form reports for act none and leaky with a slope in (0, 1]; ReLU and other slopes
# turn the two rows forms into MFMA (expected_form below).
Case = collections.namedtuple("Case", "name form dtype B C H W d s2 f_cstride y_cstride y_coff")


def _dd(d, s2):
    D = 2 * (d // s2) + 1
    return D * D


def _rows64():
    out = []
    for (B, H, W) in ((1, 1, 1),      # the odd column parity has no pixel, row parity 1 has no row
                      (1, 2, 2),
                      (2, 5, 3),
                      (1, 7, 64),     # full width; 4 row groups, the last one ragged
                      (3, 7, 63),     # 12 workgroups: XCD remap with remainder 4
                      (1, 4, 33)):
        for fcs in (256, 288):
            out.append(Case(f"rows64_{B}x{H}x{W}_f{fcs}", ROWS64, F16, B, 256, H, W, 20, 2, fcs, 464, 8))
    out.append(Case("rows64_2x5x3_y448_0", ROWS64, F16, 2, 256, 5, 3, 20, 2, 256, 448, 0))    # the slice ends 7 short of the pitch
    out.append(Case("rows64_1x7x64_y480_32", ROWS64, F16, 1, 256, 7, 64, 20, 2, 256, 480, 32))  # FlowNetC's concat slice
    return out


def _rows():
    out = []
    for (B, H, W, ycs, yco) in ((1, 3, 65, 464, 8),      # the second column chunk holds one pixel
                                (2, 7, 129, 464, 8),     # three chunks
                                (1, 2, 5, 445, 3),       # the unaligned route at small W
                                (1, 1, 64, 448, 4)):
        for fcs in (256, 288):
            out.append(Case(f"rows_{B}x{H}x{W}_f{fcs}", ROWS, F16, B, 256, H, W, 20, 2, fcs, ycs, yco))
    return out


def _mfma():
    out = []
    for (d, B, H, W) in ((0, 1, 3, 5),       # D = 1
                         (2, 2, 9, 70),
                         (4, 1, 5, 66),
                         (30, 1, 4, 40),
                         (32, 1, 5, 131)):   # window exactly 128 columns, D*D = 1089
        for fcs in (256, 264):
            out.append(Case(f"mfma_d{d}_{B}x{H}x{W}_f{fcs}", MFMA, F16, B, 256, H, W, d, 2, fcs, _dd(d, 2) + 8, 3))
    return out


def _valu():
    out = []
    # fp16: 32-pixel tiles
    for (C, d, s2) in ((8, 4, 1),
                       (64, 5, 2),       # displacement not a multiple of the stride
                       (64, 6, 3),
                       (264, 20, 2),     # C 256 + 8 must not take the matrix-core route
                       (16, 0, 1)):
        for (W, B, H, gap) in ((31, 1, 3, 0), (32, 1, 2, 8), (33, 2, 2, 0), (70, 1, 3, 8)):
            out.append(Case(f"valu16_c{C}_d{d}_s{s2}_{B}x{H}x{W}_f{C + gap}", VALU, F16, B, C, H, W, d, s2, C + gap,
                            _dd(d, s2) + 8, 3))
    # C 256 with an odd displacement: same drad as FlowNetC's, but not the matrix-core route.  (C 256, d 34, s2 2 - a
    # displacement above 32 - needs 226 496 B of LDS in this form and is in REFUSED.)
    out.append(Case("valu16_c256_d21_s2_1x3x33_f264", VALU, F16, 1, 256, 3, 33, 21, 2, 264, 441 + 8, 3))
    # fp32: 16-pixel tiles
    for (C, d, s2) in ((8, 3, 1), (24, 4, 2)):
        for (W, B, H, gap) in ((15, 1, 3, 0), (16, 1, 2, 8), (17, 2, 2, 0), (40, 1, 3, 8)):
            out.append(Case(f"valu32_c{C}_d{d}_s{s2}_{B}x{H}x{W}_f{C + gap}", VALU, F32, B, C, H, W, d, s2, C + gap,
                            _dd(d, s2) + 8, 3))
    out.append(Case("valu32_c256_d20_s2_1x5x17_f256", VALU, F32, 1, 256, 5, 17, 20, 2, 256, 480, 32))   # LDS above 64 KiB
    return out


CASES = _rows64() + _rows() + _mfma() + _valu()

# -1 from the query, FT_ERR_UNSUPPORTED from the launch, y untouched: the VALU form's LDS budget of 163 840 B
REFUSED = [
    Case("refused_fp32_c512_d20", -1, F32, 1, 512, 3, 17, 20, 2, 512, 448, 0),        # 176 832 B
    Case("refused_fp16_c512_d20", -1, F16, 1, 512, 3, 33, 20, 2, 512, 448, 0),        # 164 608 B, just over
    Case("refused_fp16_c64_d20_s1", -1, F16, 1, 64, 3, 33, 20, 1, 64, 1688, 0),
    Case("refused_fp16_c256_d34", -1, F16, 1, 256, 3, 33, 34, 2, 256, 1232, 0),       # 226 496 B: D*D = 1225 alone takes 156 800
]
# -1 from the query, FT_ERR_INVALID_ARG from the launch
INVALID = [
    Case("invalid_c_mod_8", -1, F16, 1, 12, 3, 5, 4, 2, 16, 32, 0),
    Case("invalid_f_cstride_below_c", -1, F16, 1, 256, 3, 5, 20, 2, 248, 448, 0),
    Case("invalid_slice_past_pitch", -1, F16, 1, 256, 3, 5, 20, 2, 256, 448, 8),
]


def expected_form(case, act, slope):
    """The rows kernels fold the activation into max(v, k v): they serve act none and leaky slopes in (0, 1] only (k = 0 turns a
    -inf sum into max(-inf, NaN) = -inf)."""
    if case.form in (ROWS, ROWS64) and (act == RELU or (act == LEAKY and not 0.0 < slope <= 1.0)):
        return MFMA
    return case.form


def first_of(form, dtype=F16):
    return next(c for c in CASES if c.form == form and c.dtype == dtype)


def by_name(name):
    return next(c for c in CASES + REFUSED + INVALID if c.name == name)


def torch_dtype(case):
    return torch.float16 if case.dtype == F16 else torch.float32


def data_key(case):
    """Rows that differ only in pitches and offsets see the same feature values, and share one reference."""
    return (case.dtype, case.B, case.C, case.H, case.W, case.d, case.s2)


def make_features(case, seed=11):
    """f1, f2: CPU tensors [B, H, W, f_cstride] of the row's dtype, N(0, 1) in the first C channels (rounded to fp16 first when
    the dtype is fp16, so a reference sees the operands the kernel sees), NaN in the gap channels behind them."""
    out = []
    for which in ("a", "b"):
        tag = "corr_forms_%s_%d_%dx%dx%dx%d" % (which, case.dtype, case.B, case.H, case.W, case.C)
        v = synth.normal(seed, tag, (case.B, case.H, case.W, case.C)).to(torch_dtype(case))
        f = torch.full((case.B, case.H, case.W, case.f_cstride), float("nan"), dtype=torch_dtype(case))
        f[..., :case.C] = v
        out.append(f)
    return out


_REFERENCE = {}


def reference(case):
    """(raw, S) of correlation_ref.correlation_nhwc_ref without activation, float64 [B, H, W, D*D]; computed once per data_key,
    never modified by its users (the activation is applied to a copy: correlation_ref.activation)."""
    key = data_key(case)
    if key not in _REFERENCE:
        f1, f2 = make_features(case)
        _REFERENCE[key] = correlation_nhwc_ref(f1, f2, case.C, case.d, case.s2, NONE, 0.0)
    return _REFERENCE[key]
