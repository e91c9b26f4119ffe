"""Host side of the transposed form of ft_conv_direct (ConvTranspose2d(4, 2, 1) on whole small maps as one GEMM + col2im): which
descriptors the plan accepts, the stream id and byte count — the library loads without a GPU — and the check that the error
bound of the GPU test holds for a plain sequential fp32 evaluation."""
import ctypes

import pytest
import torch

from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd._lib import ConvDesc

import deconv_direct_cases as cases


def _desc(N, Hi, Wi, Cin, Cout, /, **kw):
    d = ConvDesc()
    d.dtype = _lib.FT_F16
    d.N, d.Hi, d.Wi, d.Cin, d.Cout = N, Hi, Wi, Cin, Cout
    d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = Cin, 0, Cout, 0
    d.kh = d.kw = 4
    d.stride, d.pad, d.transposed = 2, 1, 1
    d.Ho, d.Wo = 2 * Hi, 2 * Wi
    d.out_layout = _lib.FT_LAYOUT_NHWC
    d.act = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_plan_accepts_the_pose_head_and_the_test_shapes(hip_lib):
    shapes = [(64, 8, 6, 2048, 256)] + [c[1:6] for c in cases.CASES]
    for N, Hi, Wi, Cin, Cout in shapes:
        d = _desc(N, Hi, Wi, Cin, Cout)
        assert hip_lib.ft_conv_direct_supported(ctypes.byref(d)) == 0, (N, Hi, Wi, Cin, Cout)
        assert hip_lib.ft_conv_direct_weight_bytes(ctypes.byref(d)) == 32 * Cin * Cout     # sixteen taps of Cin x Cout fp16 weights
        assert hip_lib.ft_conv_direct_stream_id(ctypes.byref(d)) > 0
    d = _desc(3, 8, 6, 256, 48, x_cstride=256 + 32, x_coff=32, y_cstride=48 + 64, y_coff=64)
    assert hip_lib.ft_conv_direct_supported(ctypes.byref(d)) == 0


@pytest.mark.parametrize("what, d", [
    ("12x9 map (108 pixels)", dict(Hi=12, Wi=9, Ho=24, Wo=18)),
    ("Cout 24", dict(Cout=24, y_cstride=24)),
    ("Cin 96", dict(Cin=96, x_cstride=96)),
    ("residual", dict(has_residual=1, res_cstride=256)),
    ("fused tail", dict(tail_cout=17)),
    ("fp32", dict(dtype=_lib.FT_F32)),
    ("kernel 3", dict(kh=3, kw=3)),
    ("second input", dict(x2_cin=256, x2_hi=16, x2_wi=12, x2_cstride=256, x2_stride=1)),
    ("NCHW fp32 output", dict(out_layout=_lib.FT_LAYOUT_NCHW_F32)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_plan_refuses(hip_lib, what, d):
    desc = _desc(64, 8, 6, 2048, 256, **d)
    assert hip_lib.ft_conv_direct_supported(ctypes.byref(desc)) != 0, what
    assert hip_lib.ft_conv_direct_stream_id(ctypes.byref(desc)) < 0
    assert hip_lib.ft_conv_direct_weight_bytes(ctypes.byref(desc)) == 0


def test_stream_id_is_its_own(hip_lib):
    """A 1x1 layer of the same Cin / Cout orders its fragments differently: the ids must differ, and the transposed form's id must
    not depend on the batch or the map (one stream serves every batch bucket)."""
    t = _desc(64, 8, 6, 2048, 256)
    one = _desc(64, 8, 6, 2048, 256, kh=1, kw=1, stride=1, pad=0, transposed=0, Ho=8, Wo=6)
    assert hip_lib.ft_conv_direct_supported(ctypes.byref(one)) == 0
    ids = {hip_lib.ft_conv_direct_stream_id(ctypes.byref(v)) for v in (t, _desc(8, 8, 6, 2048, 256), _desc(16, 4, 3, 2048, 256))}
    assert len(ids) == 1 and hip_lib.ft_conv_direct_stream_id(ctypes.byref(one)) not in ids
    assert hip_lib.ft_conv_direct_stream_id(ctypes.byref(_desc(64, 8, 6, 256, 256))) not in ids


@pytest.mark.parametrize("name", cases.IDS)
def test_sequential_fp32_stays_inside_the_bound(name):
    """The bound of the GPU test is worst-case fp32 accumulation (x 2 for the order inside an MFMA): a plain sequential fp32 sum of
    the same exact products, scaled, shifted and rounded to fp16, has to stay inside 1 x that bound for every case."""
    r = cases.reference(name)
    got = cases.sequential_fp32(r["x"], r["w"], r["scale"], r["shift"])
    ratio = ((got - r["want"]).abs() / r["bound"]).max().item()
    print(f"{name}: sequential fp32 max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0
