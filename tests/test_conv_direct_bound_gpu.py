"""ft_conv_direct_fwd, one case per form, against float64 under a derived per-element bound (conv_bound.derived_bound: worst-case fp32
accumulation, the fp32 operations of the epilogue, one rounding to fp16 — no tuned tolerance), the implicit GEMM on the same inputs
under the same bound, the two forms against each other under the sum of their bounds, and an impulse case per tap geometry that a
wrong tap map, phase or image offset fails exactly.  Integer data (test_conv_exact_gpu.py) cannot see a precision loss; this can:
test_conv_direct_bound_cpu.py shows which degraded evaluations leave the bound.  The transposed form has test_deconv_direct_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import hip_ops, synth
from flowtrack.pytorch_amd.hip_ops import FusedConv, FusedShortcutConv
from util import make_program, run_program, view_to_nchw

import direct_bound_cases as dc
import exact_cases as ec

pytestmark = pytest.mark.gpu

DEV, F16 = torch.device("cuda:0"), torch.float16


def _run(layer, views, out_shape, ycs, yoff, direct, igemm_call, monkeypatch, residual=None):
    monkeypatch.setattr(hip_ops, "CONV_DIRECT", direct)
    monkeypatch.setattr(hip_ops, "_TILE_CACHE", {})
    monkeypatch.setattr(hip_ops, "CONV_DIRECT_MAX_PIXELS", 1 << 20)
    N, C, H, W = out_shape
    y = ec.output_view(N, H, W, C, F16, DEV, ycs, yoff)
    prog = make_program()
    if residual is not None:
        layer.record(prog, *views, y, residual=residual)
    else:
        layer.record(prog, *views, y)
    prog.resolve_choices()          # recorded as [direct | implicit GEMM]: keep the first form
    assert prog.calls[0][0] == ("ft_conv_direct_fwd" if direct else igemm_call), prog.calls[0][0]
    run_program(prog)
    ec.assert_guards(y, "direct" if direct else "implicit GEMM")
    return prog, view_to_nchw(y).double()


@pytest.mark.parametrize("name", dc.NAMES)
def test_direct_form_is_inside_the_derived_bound(hip_lib, name, monkeypatch):
    r = dc.reference(name)
    want, bound = r["want"], r["bound"]
    if r["kind"] == "shortcut":
        cout = want.shape[1]
        layer = FusedShortcutConv(r["w3"], r["bn3"], r["wd"], r["bnd"], r["stride"], dtype=F16, device=DEV, act="relu", label=name)
        views = (ec.input_view(r["t2"], F16, DEV), ec.input_view(r["x"], F16, DEV, cstride=r["x"].shape[1] + 32, coff=32))
        ycs, yoff, k, form, igemm_call, rv = cout + 64, 32, 1, "k1", "ft_conv2d_fwd", None
    else:
        c = r["case"]
        layer = FusedConv(r["w"], stride=c["s"], pad=c["p"], bias=r["bias"], bn=r["bn"], act=c["act"], slope=dc.SLOPE if c["act"] == "leaky" else 0.0,
                          dtype=F16, device=DEV, label=name)
        (xcs, xoff), (ycs, yoff) = ec.direct_offsets(c)
        views = (ec.input_view(r["x"], F16, DEV, cstride=xcs, coff=xoff),)
        rv = ec.input_view(r["res"], F16, DEV) if r["res"] is not None else None
        k, form, igemm_call = c["k"], c["form"], "ft_conv2d_fwd_ws"
    prog, got = _run(layer, views, want.shape, ycs, yoff, True, igemm_call, monkeypatch, rv)
    sid = int(hip_lib.ft_conv_direct_stream_id(prog.conv_records[0][3]))
    assert ec.direct_form(sid, k, False) == form, f"{name}: stream id {sid:#x}"
    _, ig = _run(layer, views, want.shape, ycs, yoff, False, igemm_call, monkeypatch, rv)
    ratio = ((got - want).abs() / bound).max().item()
    ratio_ig = ((ig - want).abs() / bound).max().item()
    cross = ((got - ig).abs() / (2 * bound)).max().item()
    print(f"{name} ({form}, K = {r['K']}): max |err| / bound: direct {ratio:.4f}, implicit GEMM {ratio_ig:.4f}; |direct - igemm| / (sum of bounds) {cross:.4f}; "
          f"elements that differ between the forms: {(got != ig).double().mean().item():.5f}")
    assert ratio <= 1.0, f"{name}: direct form outside the bound, max |err| / bound = {ratio:.3f}"
    assert ratio_ig <= 1.0, f"{name}: implicit GEMM outside the bound, max |err| / bound = {ratio_ig:.3f}"
    assert cross <= 1.0, f"{name}: direct vs implicit GEMM outside the sum of their bounds ({cross:.3f})"


@pytest.mark.parametrize("case", dc.IMPULSES, ids=[c[0] for c in dc.IMPULSES])
def test_impulse_is_exact(hip_lib, case, monkeypatch):
    """One non-zero input pixel at the first corner of the first image and one at the last corner of the last image, no BN, no
    activation: every output element is a single product w * 1 or w * 2, exact in fp16."""
    name, N, Cin, H, W, Cout, k, s, p, form = case
    w = synth.normal(dc.SEED, name + ".w", (Cout, Cin, k, k)).half().float()
    x = dc.impulse_input(N, Cin, H, W)
    want = F.conv2d(x.double(), w.double(), stride=s, padding=p)
    assert int((want != 0).sum()) >= 2 * Cout
    c = dict(Cin=Cin, Cout=Cout, k=k, tr=False, xoff=32)
    (xcs, xoff), (ycs, yoff) = ec.direct_offsets(c)
    layer = FusedConv(w, stride=s, pad=p, dtype=F16, device=DEV, label=name)
    views = (ec.input_view(x, F16, DEV, cstride=xcs, coff=xoff),)
    prog, got = _run(layer, views, want.shape, ycs, yoff, True, "ft_conv2d_fwd_ws", monkeypatch)
    sid = int(hip_lib.ft_conv_direct_stream_id(prog.conv_records[0][3]))
    assert ec.direct_form(sid, k, False) == form, f"{name}: stream id {sid:#x}"
    ec.assert_exact(got, want, f"{name} ({form} form)")
    _, ig = _run(layer, views, want.shape, ycs, yoff, False, "ft_conv2d_fwd_ws", monkeypatch)
    ec.assert_exact(ig, want, f"{name} (implicit GEMM)")


def test_shortcut_impulse_is_exact(hip_lib, monkeypatch):
    """The K-concatenated GEMM with a stride-2 second input: t2 is non-zero at the first corner of the first image and the last corner
    of the last, x at the last corner of the first image and the first corner of the last (other output pixels, so every element stays
    a single product); both BatchNorms are the identity."""
    name, N, Hx, Wx, planes, cin_x, s = dc.IMPULSE_SHORTCUT
    cout = 4 * planes
    H, W = (Hx - 1) // s + 1, (Wx - 1) // s + 1
    w3 = synth.normal(dc.SEED, name + ".w3", (cout, planes, 1, 1)).half().float()
    wd = synth.normal(dc.SEED, name + ".wd", (cout, cin_x, 1, 1)).half().float()
    ident = lambda: {"weight": torch.ones(cout), "bias": torch.zeros(cout), "running_mean": torch.zeros(cout), "running_var": torch.ones(cout), "eps": 0.0}
    t2 = dc.impulse_input(N, planes, H, W)
    x = torch.zeros((N, cin_x, Hx, Wx))
    x[0, cin_x - 1, Hx - 1, Wx - 1] = 2.0
    x[N - 1, 3, 0, 0] = 1.0
    assert (Hx - 1) % s == 0 and (Wx - 1) % s == 0, "the last corner of x is a sampled pixel"
    want = F.conv2d(t2.double(), w3.double()) + F.conv2d(x.double(), wd.double(), stride=s)
    assert int((want != 0).sum()) >= 4 * cout - 8
    layer = FusedShortcutConv(w3, ident(), wd, ident(), s, dtype=F16, device=DEV, act=None, label=name)
    views = (ec.input_view(t2, F16, DEV), ec.input_view(x, F16, DEV, cstride=cin_x + 32, coff=32))
    prog, got = _run(layer, views, want.shape, cout + 64, 32, True, "ft_conv2d_fwd", monkeypatch)
    assert ec.direct_form(int(hip_lib.ft_conv_direct_stream_id(prog.conv_records[0][3])), 1, False) == "k1"
    ec.assert_exact(got, want, f"{name} (direct)")
    _, ig = _run(layer, views, want.shape, cout + 64, 32, False, "ft_conv2d_fwd", monkeypatch)
    ec.assert_exact(ig, want, f"{name} (implicit GEMM)")
