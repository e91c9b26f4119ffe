"""Backward of Correlation / Resample2d / ChannelNorm on the GPU (ft_*_bwd through flownet.ops) against the float64
restatements of tests/flow_grad_ref.py: per-op gradients, gradient subsets, run-to-run determinism, graph capture, and a
small FlowNetC-shaped graph end to end."""
import ctypes

import numpy as np
import pytest
import torch

import flow_grad_ref as ref
from flowtrack.pytorch_amd import synth
from flowtrack.pytorch_amd._lib import check
from flowtrack.pytorch_amd.flownet import ops

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

# B, C, H, W, pad, k, max_disp, s1, s2: CORR_CASES of test_flow_gpu.py, then FlowNetC's parameters at its 48 x 64 map
CORR_CASES = [
    (2, 16, 12, 14, 4, 1, 4, 1, 2),
    (1, 256, 12, 16, 20, 1, 20, 1, 2),
    (1, 8, 10, 9, 3, 3, 2, 1, 1),
    (1, 8, 16, 15, 4, 1, 4, 2, 2),
    (1, 5, 9, 11, 2, 1, 3, 1, 1),
    (2, 256, 48, 64, 20, 1, 20, 1, 2),
    # fast-path boundaries: stride2 4 (128-pixel tiles, four residue classes) at drad 1, 9 and 10, stride2 1 at drad 1 and 10,
    # channel counts that leave a partial chunk; stride2 3 takes the gather kernel
    (2, 12, 11, 37, 6, 1, 7, 1, 4),
    (1, 8, 10, 140, 36, 1, 36, 1, 4),
    (1, 40, 9, 150, 43, 1, 43, 1, 4),
    (1, 20, 9, 40, 1, 1, 1, 1, 1),
    (1, 130, 14, 45, 10, 1, 10, 1, 1),
    (1, 6, 9, 13, 6, 1, 6, 1, 3),
]


def _close(got, want, what=""):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= 1e-4 * max(scale, 1e-30), f"{what}: max abs err {err:.3e} vs max |ref| {scale:.3e}"


def _ref_grads(fn, inputs, g):
    leaves = [t.detach().double().cpu().requires_grad_() for t in inputs]
    fn(*leaves).backward(g.detach().double().cpu())
    return [t.grad for t in leaves]


def _gpu_grads(fn, inputs, g, need=None):
    leaves = [t.detach().cuda().requires_grad_(need is None or i in need) for i, t in enumerate(inputs)]
    fn(*leaves).backward(g.cuda())
    torch.cuda.synchronize()
    return [t.grad for t in leaves]


def _corr_case(case):
    B, C, H, W, pad, k, md, s1, s2 = case
    a = synth.normal(21, f"a{case}", (B, C, H, W))
    b = synth.normal(21, f"b{case}", (B, C, H, W))
    with torch.no_grad():
        shape = ref.correlation_fwd(a[:, :1], b[:, :1], pad, k, md, s1, s2).shape
    g = synth.normal(21, f"g{case}", (B,) + tuple(shape[1:]))
    return a, b, g, (pad, k, md, s1, s2)


@pytest.mark.parametrize("case", CORR_CASES, ids=[str(c) for c in CORR_CASES])
def test_correlation_grad_matches_float64(case):
    a, b, g, p = _corr_case(case)
    want = _ref_grads(lambda x, y: ref.correlation_fwd(x, y, *p), (a, b), g)
    got = _gpu_grads(lambda x, y: ops.CorrelationFunction.apply(x, y, *p), (a, b), g)
    _close(got[0], want[0], "grad_in1")
    _close(got[1], want[1], "grad_in2")


def _flows(kind, B, H, W, tag):
    if kind == "smooth":
        return synth.flow_field(22, B, H, W, magnitude=6.0)
    if kind == "noise":
        return synth.normal(22, f"n{tag}", (B, 2, H, W)) * 4.0
    if kind == "far":
        f = synth.normal(22, f"f{tag}", (B, 2, H, W)) * 4.0
        far = synth.uniform(22, f"s{tag}", (B, 1, H, W)) < 0.05
        f = torch.where(far, f * 6.0, f)
        f[B - 1] = synth.normal(22, f"w{tag}", (2, H, W)) * 60.0                   # spread over the whole map
        f[0, :, 0, 0] = torch.tensor([-1000.0, 2500.0])
        return f
    f = synth.flow_field(22, B, H, W, magnitude=3.0)                               # "huge": 1e9 vectors among ordinary ones
    f[0, :, 0, 0] = torch.tensor([1e9, -1e9])
    f[B - 1, :, H - 1, W - 1] = torch.tensor([-1e9, 1e9])
    f[0, :, H // 2, :] = torch.tensor([1e9, 0.0]).view(2, 1)
    return f


RS_CASES = [(2, 1, 37, 75, "smooth"), (1, 2, 33, 130, "noise"), (2, 3, 70, 150, "far"), (1, 4, 16, 64, "huge"),
            (2, 7, 21, 33, "noise"), (1, 3, 96, 256, "smooth"), (2, 3, 40, 67, "far")]


@pytest.mark.parametrize("case", RS_CASES, ids=[str(c) for c in RS_CASES])
def test_resample2d_grad_matches_float64(case):
    B, C, H, W, kind = case
    img = synth.normal(23, f"i{case}", (B, C, H, W))
    flow = _flows(kind, B, H, W, str(case))
    g = synth.normal(23, f"g{case}", (B, C, H, W))
    want = _ref_grads(ref.resample2d_fwd, (img, flow), g)
    got = _gpu_grads(ops.Resample2dFunction.apply, (img, flow), g)
    assert torch.isfinite(got[1]).all()
    _close(got[0], want[0], "grad_in1")
    _close(got[1], want[1], "grad_flow")


@pytest.mark.parametrize("shape", [(2, 3, 12, 20), (1, 5, 7, 9), (3, 1, 4, 4), (2, 2, 48, 64)])
def test_channelnorm_grad_matches_float64(shape):
    B, C, H, W = shape
    x = synth.normal(24, f"x{shape}", shape)
    x[0, :, 1, 1] = 0.0
    x[B - 1, :, H - 1, :] = 0.0
    g = synth.normal(24, f"g{shape}", (B, 1, H, W))
    want = _ref_grads(ref.channelnorm_fwd, (x,), g)
    got = _gpu_grads(ops.ChannelNormFunction.apply, (x,), g)
    assert torch.isfinite(got[0]).all() and float(got[0][0, :, 1, 1].abs().max()) == 0.0
    _close(got[0], want[0], "grad_in1")


@pytest.mark.parametrize("case", [CORR_CASES[0], (1, 40, 9, 150, 43, 1, 43, 1, 4)], ids=["s2=2", "s2=4"])
def test_needs_input_grad_subsets(case):
    a, b, g, p = _corr_case(case)
    corr = lambda x, y: ops.CorrelationFunction.apply(x, y, *p)  # noqa: E731
    only = {i: _gpu_grads(corr, (a, b), g, need={i}) for i in (1, 0)}
    both = _gpu_grads(corr, (a, b), g)
    for i in (0, 1):
        assert only[i][1 - i] is None and torch.equal(only[i][i], both[i])
    if case != CORR_CASES[0]:
        return
    img = synth.normal(25, "si", (2, 3, 40, 67))
    flow = _flows("noise", 2, 40, 67, "subset")
    gr = synth.normal(25, "sg", (2, 3, 40, 67))
    both = _gpu_grads(ops.Resample2dFunction.apply, (img, flow), gr)
    only_flow = _gpu_grads(ops.Resample2dFunction.apply, (img, flow), gr, need={1})
    assert only_flow[0] is None and torch.equal(only_flow[1], both[1])
    only_img = _gpu_grads(ops.Resample2dFunction.apply, (img, flow), gr, need={0})
    assert only_img[1] is None
    torch.testing.assert_close(only_img[0], both[0], rtol=1e-6, atol=1e-6 * float(both[0].abs().max()))


def test_backward_is_deterministic():
    a, b, g, p = _corr_case((2, 256, 48, 64, 20, 1, 20, 1, 2))
    corr = lambda x, y: ops.CorrelationFunction.apply(x, y, *p)  # noqa: E731
    r1, r2 = _gpu_grads(corr, (a, b), g), _gpu_grads(corr, (a, b), g)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    img = synth.normal(26, "di", (4, 3, 96, 128))
    flow = _flows("noise", 4, 96, 128, "det")
    gr = synth.normal(26, "dg", (4, 3, 96, 128))
    r1 = _gpu_grads(ops.Resample2dFunction.apply, (img, flow), gr)
    r2 = _gpu_grads(ops.Resample2dFunction.apply, (img, flow), gr)
    assert torch.equal(r1[1], r2[1])
    assert float((r1[0] - r2[0]).abs().max()) <= 1e-6 * float(r1[0].abs().max())
    x = synth.normal(26, "dx", (4, 3, 96, 128))
    gn = synth.normal(26, "dn", (4, 1, 96, 128))
    r1, r2 = _gpu_grads(ops.ChannelNormFunction.apply, (x,), gn), _gpu_grads(ops.ChannelNormFunction.apply, (x,), gn)
    assert torch.equal(r1[0], r2[0])


def test_backward_calls_replay_in_a_graph(hip_lib):
    a, b, g, p = (t.cuda() if isinstance(t, torch.Tensor) else t for t in _corr_case(CORR_CASES[0]))
    B, C, H, W = a.shape
    img = synth.normal(27, "gi", (2, 3, 40, 67)).cuda()
    flow = _flows("far", 2, 40, 67, "graph").cuda()
    gr = synth.normal(27, "gg", (2, 3, 40, 67)).cuda()
    x = synth.normal(27, "gx", (2, 3, 40, 68)).cuda()
    nrm = torch.sqrt((x * x).sum(1, keepdim=True))
    gn = synth.normal(27, "gn", (2, 1, 40, 68)).cuda()
    outs = [torch.full_like(a, 7.0), torch.full_like(b, 7.0), torch.full_like(img, 7.0), torch.full_like(flow, 7.0),
            torch.full_like(x, 7.0)]
    side = torch.cuda.Stream()
    sh = ctypes.c_void_p(side.cuda_stream)

    def calls():
        check(hip_lib.ft_correlation_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), B, C, H, W,
                                         *p, 1, sh))
        check(hip_lib.ft_resample2d_bwd(img.data_ptr(), flow.data_ptr(), gr.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), 2, 3,
                                        40, 67, sh))
        check(hip_lib.ft_channelnorm_bwd(x.data_ptr(), nrm.data_ptr(), gn.data_ptr(), outs[4].data_ptr(), 2, 3, 40, 68, sh))

    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    calls()                                                      # eager, also raises the LDS limits before capture
    check(hip_lib.ft_stream_synchronize(sh))
    eager = [o.clone() for o in outs]
    for o in outs:
        o.fill_(7.0)
    torch.cuda.synchronize()
    check(hip_lib.ft_graph_begin_capture(sh))
    try:
        calls()
    finally:
        exec_ = ctypes.c_void_p()
        st = hip_lib.ft_graph_end_capture(sh, ctypes.byref(exec_))
    check(st)
    try:
        for _ in range(2):
            check(hip_lib.ft_graph_launch(exec_, sh))
        check(hip_lib.ft_stream_synchronize(sh))
    finally:
        check(hip_lib.ft_graph_destroy(exec_))
    for i, (o, e) in enumerate(zip(outs, eager)):
        if i == 2:                                               # Resample2d grad_in1: float atomics
            assert float((o - e).abs().max()) <= 1e-6 * float(e.abs().max()), i
        else:
            assert torch.equal(o, e), i


def test_flownetc_shaped_graph_end_to_end():
    """1x1 projections (einsum) of two frames -> Correlation(4,1,4,1,2) -> LeakyReLU(0.1) -> einsum to a 2-channel flow ->
    Resample2d(img2, flow) -> ChannelNorm(img1 - warped) -> mean; fp32 on the GPU against float64 on the CPU."""
    B, H, W, F = 2, 24, 32, 16
    img1 = synth.normal(28, "e1", (B, 3, H, W))
    img2 = synth.normal(28, "e2", (B, 3, H, W))
    w_proj = synth.normal(28, "wp", (F, 3), std=0.5)
    w_flow = synth.normal(28, "wf", (2, 25), std=4.0)

    def net(i1, i2, wp, wf, corr, resample, cnorm):
        f1 = torch.einsum("fc,bchw->bfhw", wp, i1)
        f2 = torch.einsum("fc,bchw->bfhw", wp, i2)
        c = torch.nn.functional.leaky_relu(corr(f1, f2), 0.1)
        flow = torch.einsum("od,bdhw->bohw", wf, c)
        warped = resample(i2, flow)
        return cnorm(i1 - warped).mean()

    leaves64 = [t.double().requires_grad_() for t in (img1, img2, w_proj, w_flow)]
    net(*leaves64, lambda x, y: ref.correlation_fwd(x, y, 4, 1, 4, 1, 2), ref.resample2d_fwd, ref.channelnorm_fwd).backward()
    leaves = [t.cuda().requires_grad_() for t in (img1, img2, w_proj, w_flow)]
    loss = net(*leaves, ops.Correlation(4, 1, 4, 1, 2), ops.Resample2d(), ops.ChannelNorm())
    loss.backward()
    torch.cuda.synchronize()
    for name, got, want in zip(("img1", "img2", "w_proj", "w_flow"), leaves, leaves64):
        g, w = got.grad.double().cpu(), want.grad
        err = float((g - w).abs().max())
        assert err <= 1e-4 * float(w.abs().max()), f"{name}: {err:.3e} vs {float(w.abs().max()):.3e}"
