"""ft_maxpool2x2s2_fwd and ft_fc_fwd alone, through the C ABI (include/flowtrack_hip.h, csrc/vgg_ops.hip).

The pool is bit-exact (its output is one of its inputs).  The FC is checked three ways: EQUAL to the float64 reference on integer
data on which every product, partial sum and result is exact (tests/detect_vgg_ref.py: fc_exact_case; a dropped or doubled product,
a wrong slice bound or a wrong row / column of the accumulator layout changes an integer); inside conv_bound.derived_bound on
Gaussian data; and bit-equal between two calls."""
import ctypes

import numpy as np
import pytest
import torch

import detect_vgg_ref as V
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import FT_ACT_NONE, FT_ACT_RELU, FT_ERR_INVALID_ARG, FT_ERR_UNSUPPORTED, FT_F16, FT_F32, FT_OK

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.float32]
DTYPE_IDS = ["fp16", "fp32"]
SENTINEL = -77.0


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- max-pool -------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 2, 2, 8), (2, 5, 7, 8), (1, 3, 2, 16), (1, 37, 54, 64)]


def _pool(hip_lib, x, tail=64):
    """x NHWC on the device -> (pooled, the `tail` elements behind it), from a sentinel-filled buffer."""
    N, H, W, C = x.shape
    n_out = N * (H // 2) * (W // 2) * C
    buf = torch.full((n_out + tail,), SENTINEL, dtype=x.dtype, device="cuda")
    st = hip_lib.ft_maxpool2x2s2_fwd(x.data_ptr(), buf.data_ptr(), N, H, W, C, _lib.dtype_code(x.dtype), _stream())
    assert st == FT_OK
    torch.cuda.synchronize()
    return buf[:n_out].view(N, H // 2, W // 2, C).cpu().numpy(), buf[n_out:].cpu().numpy()


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("negative", [False, True], ids=["mixed", "all_negative"])
def test_maxpool_bit_exact(hip_lib, negative, dtype, shape):
    x = synth.normal(3, f"pool{shape}", shape)
    if negative:
        x = -x.abs() - 0.125
    x = x.to(dtype)
    got, tail = _pool(hip_lib, x.cuda())
    want = V.maxpool_ref(x.numpy())
    assert got.shape == want.shape
    bits = np.uint16 if dtype == torch.float16 else np.uint32
    assert np.array_equal(got.view(bits), want.view(bits))
    assert negative is False or (got < 0).all()
    assert (tail == SENTINEL).all(), "written past N*Ho*Wo*C"


def test_maxpool_refusals_on_device_buffers(hip_lib):
    x = torch.zeros((1, 4, 4, 8), dtype=torch.float16, device="cuda")
    y = torch.full((1, 2, 2, 8), SENTINEL, dtype=torch.float16, device="cuda")
    f = lambda xp, yp, N, H, W, C, dt: hip_lib.ft_maxpool2x2s2_fwd(xp, yp, N, H, W, C, dt, _stream())
    for args in ((x.data_ptr(), y.data_ptr(), 1, 1, 4, 8, FT_F16), (x.data_ptr(), y.data_ptr(), 1, 4, 1, 8, FT_F16),
                 (x.data_ptr(), y.data_ptr(), 1, 4, 4, 12, FT_F16), (x.data_ptr() + 2, y.data_ptr(), 1, 4, 4, 8, FT_F16),
                 (x.data_ptr(), y.data_ptr() + 8, 1, 4, 4, 8, FT_F16), (None, y.data_ptr(), 1, 4, 4, 8, FT_F16),
                 (x.data_ptr(), y.data_ptr(), 0, 4, 4, 8, FT_F16), (x.data_ptr(), y.data_ptr(), 1, 4, 4, 8, 5)):
        assert f(*args) == FT_ERR_INVALID_ARG, args
    assert f(x.data_ptr(), y.data_ptr(), 4, 8192, 8192, 8, FT_F16) == FT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == SENTINEL).all(), "a refused call launched"


# ---- FC -------------------------------------------------------------------------------------------------------------------------
def _fc(hip_lib, x, w, bias, relu, x_pad=0, y_pad=0):
    """x [R,K], w [N,K], bias [N] (CPU tensors) through ft_fc_pack + ft_fc_fwd with row strides K + x_pad / N + y_pad: the whole
    y buffer [R, N + y_pad] (sentinel-filled) as numpy."""
    R, K = x.shape
    N = w.shape[0]
    xb = torch.full((max(R, 1), K + x_pad), SENTINEL, dtype=torch.float16, device="cuda")
    xb[:R, :K] = x.to(torch.float16)
    yb = torch.full((max(R, 1), N + y_pad), SENTINEL, dtype=torch.float16, device="cuda")
    w16 = w.to(torch.float16).cuda().contiguous()
    wp = torch.empty_like(w16)
    assert hip_lib.ft_fc_pack(w16.data_ptr(), N, K, wp.data_ptr(), _stream()) == FT_OK
    b = bias.to(torch.float32).cuda().contiguous()
    nbytes = hip_lib.ft_fc_workspace_bytes(R, K, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    assert hip_lib.ft_fc_supported(FT_F16, R, K, N, K + x_pad, N + y_pad) == FT_OK
    st = hip_lib.ft_fc_fwd(FT_F16, xb.data_ptr(), K + x_pad, wp.data_ptr(), b.data_ptr(), yb.data_ptr(), N + y_pad, R, K, N,
                           FT_ACT_RELU if relu else FT_ACT_NONE, ws.data_ptr(), nbytes, _stream())
    assert st == FT_OK
    torch.cuda.synchronize()
    return yb.cpu().numpy(), xb.cpu().numpy()


@pytest.mark.parametrize("case", V.FC_EXACT_CASES, ids=lambda c: "R%d_K%d_N%d" % c)
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_fc_exact_integer_data(hip_lib, relu, case):
    """Strided x and y views with sentinels between the rows; the result EQUALS the float64 reference."""
    R, K, N = case
    x, w, bias = V.fc_exact_case(*case)
    pre = V.fc_exact_ref(*case)
    want = np.maximum(pre, 0.0) if relu else pre
    got, xb = _fc(hip_lib, torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias), relu, x_pad=8, y_pad=16)
    assert np.array_equal(got[:R, :N].astype(np.float64), want), f"{(got[:R, :N].astype(np.float64) != want).sum()} of {want.size} differ"
    assert (got[:, N:] == SENTINEL).all() and (xb[:, K:] == SENTINEL).all(), "written between the rows"


def test_fc_gaussian_within_derived_bound(hip_lib):
    R, K, N = 300, 4096, 256
    x = synth.normal(11, "fc_gauss.x", (R, K)).half()
    w = synth.normal(11, "fc_gauss.w", (N, K), std=float(np.sqrt(2.0 / K))).half()
    bias = synth.normal(11, "fc_gauss.b", (N,), std=0.5)
    got, _ = _fc(hip_lib, x, w, bias, True)
    bound, want, _ = V.fc_bound(x, w, bias, relu=True)
    err = (torch.from_numpy(got.astype(np.float64)) - want).abs()
    ratio = float((err / bound).max())
    print(f"fc gaussian R{R} K{K} N{N}: max abs {float(err.max()):.3e} on values of {float(want.abs().max()):.2f}, {ratio:.3f} of the derived bound")
    assert ratio <= 1.0
    again, _ = _fc(hip_lib, x, w, bias, True)
    assert np.array_equal(got.view(np.uint16), again.view(np.uint16)), "two calls on the same data differ"


def test_fc_zero_rows_and_refusals(hip_lib):
    K, N = 128, 64
    x = torch.zeros((4, K), dtype=torch.float16, device="cuda")
    wp = torch.zeros((N, K), dtype=torch.float16, device="cuda")
    b = torch.zeros(N, dtype=torch.float32, device="cuda")
    y = torch.full((4, N), SENTINEL, dtype=torch.float16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    X, W, B, Y, S = x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), ws.data_ptr()
    f = lambda dt, xp, xs, wpp, bp, yp, ys, R, k, n, act, wsp, wsb: hip_lib.ft_fc_fwd(dt, xp, xs, wpp, bp, yp, ys, R, k, n, act, wsp, wsb, _stream())
    assert f(FT_F16, None, K, None, None, None, N, 0, K, N, FT_ACT_RELU, None, 0) == FT_OK                   # zero rows: no launch
    need = hip_lib.ft_fc_workspace_bytes(4, K, N)
    assert need > 0 and hip_lib.ft_fc_workspace_bytes(0, K, N) == 0 and hip_lib.ft_fc_workspace_bytes(4, K + 8, N) == 0
    invalid = ((5, X, K, W, B, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K, W, B, Y, N, -1, K, N, 0, S, need),
               (FT_F16, X, K - 8, W, B, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K, W, B, Y, N - 8, 4, K, N, 0, S, need),
               (FT_F16, X, K + 4, W, B, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K, W, B, Y, N + 4, 4, K, N, 0, S, need),
               (FT_F16, X, K, W, B, Y, N, 4, 0, N, 0, S, need), (FT_F16, X, K, W, B, Y, N, 4, K, 0, 0, S, need),
               (FT_F16, None, K, W, B, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K, None, B, Y, N, 4, K, N, 0, S, need),
               (FT_F16, X, K, W, B, None, N, 4, K, N, 0, S, need), (FT_F16, X, K, W, B, Y, N, 4, K, N, 0, None, need),
               (FT_F16, X + 2, K, W, B, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K, W + 8, B, Y, N, 4, K, N, 0, S, need),
               (FT_F16, X, K, W, B + 4, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K, W, B, Y + 2, N, 4, K, N, 0, S, need),
               (FT_F16, X, K, W, B, Y, N, 4, K, N, 0, S + 4, need), (FT_F16, X, K, W, B, Y, N, 4, K, N, 2, S, need),
               (FT_F16, X, K, W, B, Y, N, 4, K, N, 0, S, need - 1))
    for args in invalid:
        assert f(*args) == FT_ERR_INVALID_ARG, args
    unsupported = ((FT_F32, X, K, W, B, Y, N, 4, K, N, 0, S, need), (FT_F16, X, K + 32, W, B, Y, N, 4, K + 32, N, 0, S, need),
                   (FT_F16, X, K, W, B, Y, N + 32, 4, K, N + 32, 0, S, need), (FT_F16, X, 1 << 20, W, B, Y, N, 4096, K, N, 0, S, need),
                   (FT_F16, X, 65536, W, B, Y, 32768, 4, 65536, 32768, 0, S, need))
    for args in unsupported:
        assert f(*args) == FT_ERR_UNSUPPORTED, args
        assert hip_lib.ft_fc_supported(args[0], args[7], args[8], args[9], args[2], args[6]) == FT_ERR_UNSUPPORTED
    assert hip_lib.ft_fc_pack(None, N, K, W, _stream()) == FT_ERR_INVALID_ARG and hip_lib.ft_fc_pack(X, N, K, W + 2, _stream()) == FT_ERR_INVALID_ARG
    assert hip_lib.ft_fc_pack(X, N + 32, K, W, _stream()) == FT_ERR_UNSUPPORTED and hip_lib.ft_fc_pack(X, N, K + 8, W, _stream()) == FT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == SENTINEL).all(), "a refused call launched"
