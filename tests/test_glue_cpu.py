"""The references of tests/glue_ref.py pinned on the CPU before they judge the HIP kernels (tests/test_glue_gpu.py):
against the C restatement of the reference's Resample2d / ChannelNorm (oracle/ops_ref.py), and against answers known by hand."""
import numpy as np
import pytest

import glue_ref
from oracle import ops_ref

SMALL = [s[:3] for s in glue_ref.CONCAT_SHAPES]


def _inputs(B, H, W, tag):
    x6 = glue_ref.make_images(21, f"cpu.x6.{tag}", B, H, W, fp16=False)
    flow = glue_ref.make_flow(21, f"cpu.flow.{tag}", B, H, W, fp16=False)       # with the far vectors, (1e9, -1e9) among them
    return x6, flow


def _compose_warp(x6, flow):
    return ops_ref.resample2d_c(np.ascontiguousarray(x6[:, 3:6]), flow)


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_warp_concat_ref_is_the_composition_of_the_reference_operators(oracle_lib, shape):
    B, H, W = shape
    x6, flow = _inputs(B, H, W, "w")
    warp = _compose_warp(x6, flow)
    want = np.concatenate((x6, warp, flow / np.float32(glue_ref.DIV_FLOW), ops_ref.channelnorm_c(x6[:, :3] - warp)), axis=1)
    got = glue_ref.warp_concat_ref(x6, flow, glue_ref.DIV_FLOW)
    assert got.dtype == np.float64 and got.shape == (B, 12, H, W)
    assert np.abs(got - want).max() <= 1e-5


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_fusion_concat_ref_is_the_composition_of_the_reference_operators(oracle_lib, shape):
    B, H, W = shape
    x6, fsd = _inputs(B, H, W, "sd")
    fs2 = glue_ref.make_flow(22, "cpu.flow.s2", B, H, W, fp16=True)
    img0 = x6[:, :3]
    want = np.concatenate((img0, fsd, fs2, ops_ref.channelnorm_c(fsd), ops_ref.channelnorm_c(fs2),
                           ops_ref.channelnorm_c(img0 - _compose_warp(x6, fsd)), ops_ref.channelnorm_c(img0 - _compose_warp(x6, fs2))), axis=1)
    got = glue_ref.fusion_concat_ref(x6, fsd, fs2)
    assert got.dtype == np.float64 and got.shape == (B, 11, H, W)
    # every channel to 1e-5, except |flow| where the fp32 oracle cannot resolve 1e-5: its sqrt(x*x + y*y) carries 2^-23 of the
    # value (two roundings under the root count half, one behind it), which is 3e-5 at 250 px and 170 at the (1e9, -1e9) vector
    err = np.abs(got - want)
    bound = np.full_like(err, 1e-5)
    bound[:, 7:9] = np.maximum(1e-5, np.abs(got[:, 7:9]) * 2.0 ** -23)
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_zero_flow_is_the_identity_and_integer_flow_a_shift(shape):
    B, H, W = shape
    x6, _ = _inputs(B, H, W, "id")
    img1 = x6[:, 3:6].astype(np.float64)
    zero = np.zeros((B, 2, H, W), dtype=np.float32)
    assert np.array_equal(glue_ref.warp_ref(img1, zero), img1)
    got = glue_ref.warp_concat_ref(x6, zero, glue_ref.DIV_FLOW)
    assert np.array_equal(got[:, 6:9], img1) and np.array_equal(got[:, :6], x6.astype(np.float64)) and not got[:, 9:11].any()
    assert np.abs(got[:, 11] - np.sqrt(((x6[:, :3].astype(np.float64) - img1) ** 2).sum(1))).max() <= 1e-14
    for dx, dy in ((1, -2), (-3, 1), (0, 2)):
        flow = np.empty((B, 2, H, W), dtype=np.float32)
        flow[:, 0], flow[:, 1] = dx, dy
        out = glue_ref.warp_ref(img1, flow)
        ys = np.arange(max(0, -dy), min(H, H - dy))          # pixels whose source (y + dy, x + dx) lies inside the frame
        xs = np.arange(max(0, -dx), min(W, W - dx))
        if len(ys) and len(xs):
            assert np.array_equal(out[:, :, ys[:, None], xs[None]], img1[:, :, (ys + dy)[:, None], (xs + dx)[None]])
        # outside: the border pixel (clamped index, weight 1 on it)
        yc, xc = np.clip(np.arange(H) + dy, 0, H - 1), np.clip(np.arange(W) + dx, 0, W - 1)
        assert np.array_equal(out, img1[:, :, yc[:, None], xc[None]])


def test_far_flows_clamp_to_the_border_without_renormalising():
    """A vector far out of frame lands on the clamped corner pixel with the weights of its own fractions: an integer target has
    weight 1 on one tap (all four taps are the same corner pixel anyway), so the result is that pixel — also at 1e9, where
    x + dx is far beyond any integer conversion."""
    B, H, W = 1, 5, 7
    x6, _ = _inputs(B, H, W, "far")
    img1 = x6[:, 3:6].astype(np.float64)
    for (dx, dy), (cy, cx) in (((-1000.0, 2500.0), (H - 1, 0)), ((3000.0, -3000.0), (0, W - 1)), ((1e9, -1e9), (0, W - 1)),
                               ((-1000.5, 2500.25), (H - 1, 0))):
        flow = np.empty((B, 2, H, W), dtype=np.float32)
        flow[:, 0], flow[:, 1] = dx, dy
        out = glue_ref.warp_ref(img1, flow)
        assert np.abs(out - img1[:, :, cy, cx][:, :, None, None]).max() <= 1e-12
