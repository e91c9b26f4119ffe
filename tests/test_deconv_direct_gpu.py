"""The transposed form of ft_conv_direct_fwd — ConvTranspose2d(4, 2, 1) on whole small maps as one weight-streaming GEMM whose
epilogue does the col2im (the pose head's first deconv, pose_deconv.py:43) — against torch's conv_transpose2d in float64 on the
CPU under a derived per-element bound (deconv_direct_cases.bound), against the implicit-GEMM form on the same inputs, and an
impulse case that a wrong tap map fails exactly."""
import pytest
import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import hip_ops
from flowtrack.pytorch_amd.hip_ops import ActView, FusedConv
from util import make_program, nchw_to_view, run_program, view_to_nchw

import deconv_direct_cases as cases

pytestmark = pytest.mark.gpu


def _run(conv, xv, N, Ho, Wo, Cout, y_coff, direct, monkeypatch, fill=3.0):
    monkeypatch.setattr(hip_ops, "CONV_DIRECT", direct)
    monkeypatch.setattr(hip_ops, "_TILE_CACHE", {})
    y = ActView(torch.full((N, Ho, Wo, Cout + 2 * y_coff), fill, dtype=torch.float16, device=xv.t.device), Cout, y_coff)
    prog = make_program()
    conv.record(prog, xv, y)
    prog.resolve_choices()          # recorded as [direct | implicit GEMM]: keep the first form
    assert prog.calls[0][0] == ("ft_conv_direct_fwd" if direct else "ft_conv2d_fwd_ws"), prog.calls[0][0]
    run_program(prog)
    return prog, y


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_transposed_direct_matches_float64_and_igemm(hip_lib, case, monkeypatch):
    name, N, Hi, Wi, Cin, Cout, (x_coff, y_coff) = case
    dev, dtype = torch.device("cuda:0"), torch.float16
    r = cases.reference(name)
    conv = FusedConv(r["w"], stride=2, pad=1, transposed=True, bn=r["bn"], act="relu", dtype=dtype, device=dev, label=name)
    xv = nchw_to_view(r["x"], dtype, dev, cstride=Cin + 2 * x_coff, coff=x_coff)
    prog, y = _run(conv, xv, N, 2 * Hi, 2 * Wi, Cout, y_coff, True, monkeypatch)
    got = view_to_nchw(y).double()
    if y_coff:
        assert torch.all(y.t[..., :y_coff] == 3.0) and torch.all(y.t[..., y_coff + Cout:] == 3.0), "channels outside the view were written"
    y.t.fill_(5.0)
    run_program(prog)               # determinism: a fixed summation order, no atomics
    assert torch.equal(view_to_nchw(y).double(), got)
    _, y2 = _run(conv, xv, N, 2 * Hi, 2 * Wi, Cout, y_coff, False, monkeypatch)
    ig = view_to_nchw(y2).double()
    ratio = ((got - r["want"]).abs() / r["bound"]).max().item()
    ratio_ig = ((ig - r["want"]).abs() / r["bound"]).max().item()
    cross = ((got - ig).abs() / (2 * r["bound"])).max().item()
    print(f"{name}: max |err| / bound: direct {ratio:.4f}, implicit GEMM {ratio_ig:.4f}; |direct - igemm| / (sum of bounds) {cross:.4f}; "
          f"elements that differ between the forms: {(got != ig).double().mean().item():.5f}")
    assert ratio <= 1.0, f"{name}: direct form outside the bound, max |err| / bound = {ratio:.3f}"
    assert cross <= 1.0, f"{name}: direct vs implicit GEMM outside the sum of their bounds ({cross:.3f})"


def test_transposed_direct_impulse_is_exact(hip_lib, monkeypatch):
    """One non-zero input pixel at the first corner of the first image and one at the last corner of the last image (ragged tile),
    no BN, no activation: every output element is a single product w * 1 or w * 2, exact in fp16 — a wrong (ky, kx) -> output map,
    a wrong phase / tap in the weight stream or a wrong image offset changes elements outright."""
    N, Hi, Wi, Cin, Cout = 3, 8, 6, 256, 48
    dev, dtype = torch.device("cuda:0"), torch.float16
    w = cases.synth.normal(43, "impulse.w", (Cin, Cout, 4, 4)).half().float()
    x = torch.zeros((N, Cin, Hi, Wi))
    x[0, 3, 0, 0] = 1.0
    x[N - 1, Cin - 1, Hi - 1, Wi - 1] = 2.0
    want = F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1)
    conv = FusedConv(w, stride=2, pad=1, transposed=True, dtype=dtype, device=dev, label="impulse")
    _, y = _run(conv, nchw_to_view(x, dtype, dev), N, 2 * Hi, 2 * Wi, Cout, 0, True, monkeypatch)
    got = view_to_nchw(y).double()
    assert want.abs().sum() > 0 and torch.equal(got, want), f"{(got != want).sum().item()} elements differ"
