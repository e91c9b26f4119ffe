"""The integer-data cases of test_conv_exact_gpu.py / test_bottleneck_exact_gpu.py (tests/exact_cases.py), checked on the CPU: every
value a kernel stores in fp16 is representable, nothing exceeds 2048, the activation does not hide most of the output, every weight
column / output channel / input channel takes part, and a single dropped or doubled product changes the reference (the cases have
teeth).  Also: hip_ops.fold_scale_shift returns the intended powers of two exactly, and the direct-conv cases plan to the kernel form
they are named for (the library loads without a GPU)."""
import ctypes

import pytest
import torch

from flowtrack.pytorch_amd import _lib, hip_ops
from flowtrack.pytorch_amd._lib import ConvDesc

import exact_cases as ec

ALL = ec.all_cases()


@pytest.mark.parametrize("make", [m for _, m in ALL], ids=[n for n, _ in ALL])
def test_case_is_exact_covered_and_has_teeth(make):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    chain = make()
    mx, zeros = ec.tensor_report(chain)
    last = chain.layers[-1]
    limit = 0.60 if any(L.act == "relu" for L in chain.layers if L.out in chain.outputs) else 0.05
    print(f"{chain.name}: max magnitude {mx:.1f}, zero share of the output {zeros:.3f} (limit {limit})")
    assert mx <= 2048.0
    assert zeros <= limit, f"{chain.name}: {zeros:.3f} of the outputs are zero"
    assert last.out in chain.outputs
    ec.coverage(chain)
    assert ec.teeth(chain) == 16


def test_generator_is_integer_valued_and_deterministic():
    a = ec.ints(3, "gen", (64, 33), 0.25, 3)
    assert torch.equal(a, ec.ints(3, "gen", (64, 33), 0.25, 3)) and torch.equal(a, a.round()) and a.abs().max().item() == 3
    share = (a != 0).double().mean().item()
    assert 0.2 < share < 0.3
    assert set(ec.ints(3, "gen1", (4096,), 1.0, 1).abs().unique().tolist()) == {1.0}
    w = ec.cover_weights(torch.zeros(8, 5, 3, 3, dtype=torch.float64))
    assert bool((w.abs().sum(0) > 0).all()) and bool((w.abs().sum((1, 2, 3)) > 0).all())
    x = ec.cover_input(torch.zeros(2, 7, 3, 2, dtype=torch.float64))
    assert bool((x.abs().sum((2, 3)) > 0).all())


@pytest.mark.parametrize("scales", [ec.POW2, ec.BLOCK_SCALES, ec.EXIT_SCALES], ids=["pow2", "block", "exit"])
def test_fold_scale_shift_returns_the_powers_of_two_exactly(scales):
    c = 96
    bn = ec.pow2_bn("foldcheck", c, scales)
    bias = ec.ints(ec.SEED, "foldcheck.bias", (c,), 1.0, 8).float()
    for b in (None, bias):
        scale, shift = hip_ops.fold_scale_shift(c, c + 32, b, bn, torch.device("cpu"))
        s64, sh64 = ec.fold64(c, b, bn)
        assert scale.dtype == torch.float32 and torch.equal(scale[:c].double(), bn["weight"].double()) and torch.equal(scale[:c].double(), s64)
        assert set(scale[:c].tolist()) <= set(scales) and len(set(scale[:c].tolist())) == len(set(scales))
        assert torch.equal(shift[:c].double(), sh64) and torch.equal(sh64 * 2, (sh64 * 2).round())
        assert torch.equal(scale[c:], torch.ones(32)) and torch.equal(shift[c:], torch.zeros(32))
        # folded into fp16 weights of +-1 (the shortcut conv, the strip forms): still exact
        assert torch.equal((scale[:c, None] * torch.tensor([1.0, -1.0])).half().double(), s64[:, None] * torch.tensor([1.0, -1.0]).double())


def _direct_desc(c):
    from exact_cases import out_hw
    d = ConvDesc()
    d.dtype = _lib.FT_F16
    d.N, d.Hi, d.Wi, d.Cin, d.Cout = c["N"], c["H"], c["W"], c["Cin"], c["Cout"]
    d.kh = d.kw = c["k"]
    d.stride, d.pad, d.transposed = c["s"], c["p"], int(c["tr"])
    d.Ho, d.Wo = out_hw(c["H"], c["W"], c["k"], c["s"], c["p"], c["tr"])
    xo, yo = ec.direct_offsets(c)
    d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = xo[0], xo[1], yo[0], yo[1]
    d.out_layout = _lib.FT_LAYOUT_NHWC
    d.act, d.slope = hip_ops.ACT_CODES[c["act"]], ec.SLOPE if c["act"] == "leaky" else 0.0
    if c["res"]:
        d.has_residual, d.res_cstride = 1, c["Cout"]
    return d


@pytest.mark.parametrize("c", ec.DIRECT_CONVS, ids=[c["name"] for c in ec.DIRECT_CONVS])
def test_direct_cases_plan_to_their_form(hip_lib, c):
    d = _direct_desc(c)
    assert hip_lib.ft_conv_direct_supported(ctypes.byref(d)) == 0
    sid = int(hip_lib.ft_conv_direct_stream_id(ctypes.byref(d)))
    assert ec.direct_form(sid, c["k"], c["tr"]) == c["form"], f"{c['name']}: stream id {sid:#x}"
    assert hip_lib.ft_conv_direct_weight_bytes(ctypes.byref(d)) == ec.direct_weight_bytes(c)


@pytest.mark.parametrize("c", ec.DIRECT_SHORTCUT, ids=[c[0] for c in ec.DIRECT_SHORTCUT])
def test_direct_shortcut_cases_plan_to_the_n_tile_256_form(hip_lib, c):
    _, N, Hx, Wx, planes, cin_x, s = c
    d = ConvDesc()
    d.dtype = _lib.FT_F16
    d.N, d.Hi, d.Wi = N, (Hx - 1) // s + 1, (Wx - 1) // s + 1
    d.Ho, d.Wo = d.Hi, d.Wi
    d.Cin, d.x_cstride, d.Cout, d.y_cstride, d.y_coff = planes, planes, 4 * planes, 4 * planes + 64, 32
    d.kh = d.kw = d.stride = 1
    d.out_layout, d.act = _lib.FT_LAYOUT_NHWC, hip_ops.ACT_CODES["relu"]
    d.x2_cin, d.x2_hi, d.x2_wi, d.x2_cstride, d.x2_coff, d.x2_stride = cin_x, Hx, Wx, cin_x + 32, 32, s
    assert hip_lib.ft_conv_direct_supported(ctypes.byref(d)) == 0
    assert ec.direct_form(int(hip_lib.ft_conv_direct_stream_id(ctypes.byref(d))), 1, False) == "k1"
    assert hip_lib.ft_conv_direct_weight_bytes(ctypes.byref(d)) == 2 * 4 * planes * (planes + cin_x)
