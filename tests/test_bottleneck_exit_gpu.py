"""ft_bottleneck_exit_fwd (a stage's last identity block + the 1x1 conv that opens the next stage in one launch; t1 and, of the
block's own output, all / the even pixels / nothing) vs the CPU oracle (oracle/pose_ref.py, torch CPU fp32) and vs the two launches it
replaces (ft_bottleneck_fwd, then the conv on its output), and the plan that records it vs the plan that does not."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import _lib, hip_ops, synth
from flowtrack.pytorch_amd.hip_ops import ActView, FlowtrackHipError, FusedConv, bottleneck_exit_fusable, record_bottleneck, record_bottleneck_exit
from flowtrack.pytorch_amd.pose import models
from oracle import pose_ref
from util import make_program, nchw_to_view, run_program, view_to_nchw

pytestmark = pytest.mark.gpu

P, C, T = 64, 256, 128          # planes and width of the block, output channels of the tail conv
Y_POISON, T_POISON = 3.0, 5.0

# (name, N, H, W, x channel stride, x channel offset, t1 channel stride, t1 channel offset, y mode)
CASES = [
    ("two_patch_rows_16x16", 2, 16, 16, 256, 0, 128, 0, "even"),     # 8 x 16 patches: one patch column, two patch rows
    ("ragged_24x40", 3, 24, 40, 256, 0, 128, 0, "even"),             # width divides by 8 only: 16 x 8 patches, ragged rows, odd batch
    ("ragged_cols_16x20", 2, 16, 20, 256, 0, 128, 0, "even"),        # 8 x 16 patches, the second patch column 4 pixels wide
    ("single_patch_8x16", 1, 8, 16, 256, 0, 128, 0, "even"),         # a single patch, all of its halo outside the image
    ("views_16x16", 2, 16, 16, 320, 32, 192, 32, "even"),            # x a channel slice of a wider buffer, t1 written into one
    ("y_full_16x16", 2, 16, 16, 256, 0, 128, 0, "full"),
    ("y_none_16x16", 2, 16, 16, 256, 0, 128, 0, "none"),
]


def _bn(seed, name, c):
    return {"weight": synth.uniform(seed, name + "g", (c,), 0.5, 1.5), "bias": synth.normal(seed, name + "b", (c,), 0.1),
            "running_mean": synth.normal(seed, name + "m", (c,), 0.1), "running_var": synth.uniform(seed, name + "v", (c,), 0.5, 1.5),
            "eps": 1e-5}


@functools.lru_cache(maxsize=None)
def _reference(N, H, W):
    """Layers, input, the fp32 oracle and the two launches the exit form replaces, once per shape (shared, never modified)."""
    dev, dtype, seed, name = torch.device("cuda:0"), torch.float16, 23, f"exit{N}x{H}x{W}"
    w = {"conv1": synth.normal(seed, name + ".w1", (P, C, 1, 1), std=(2.0 / C) ** 0.5),
         "conv2": synth.normal(seed, name + ".w2", (P, P, 3, 3), std=(2.0 / (9 * P)) ** 0.5),
         "conv3": synth.normal(seed, name + ".w3", (C, P, 1, 1), std=(2.0 / P) ** 0.5),
         "tail": synth.normal(seed, name + ".wt", (T, C, 1, 1), std=(2.0 / C) ** 0.5)}
    bn = {"bn1": _bn(seed, name + ".bn1", P), "bn2": _bn(seed, name + ".bn2", P), "bn3": _bn(seed, name + ".bn3", C),
          "tail": _bn(seed, name + ".bnt", T)}
    x = synth.normal(seed, name + ".x", (N, C, H, W)).half().float()
    # oracle: Bottleneck.forward as oracle/pose_ref.py states it, then the next block's conv1 + bn1 + relu
    sd = {f"b.{k}.weight": w[k] for k in ("conv1", "conv2", "conv3")}
    for k in ("bn1", "bn2", "bn3"):
        sd.update({f"b.{k}.{f}": bn[k][f] for f in ("weight", "bias", "running_mean", "running_var")})
    sd.update({f"t.{f}": bn["tail"][f] for f in ("weight", "bias", "running_mean", "running_var")})
    with torch.no_grad():
        want_y = pose_ref._bottleneck(sd, "b", x, 1)
        want_t1 = F.relu(pose_ref._bn(sd, "t", F.conv2d(want_y, w["tail"])))
    mk = dict(dtype=dtype, device=dev, act="relu")
    c1 = FusedConv(w["conv1"], bn=bn["bn1"], label="conv1", **mk)
    c2 = FusedConv(w["conv2"], pad=1, bn=bn["bn2"], label="conv2", **mk)
    c3 = FusedConv(w["conv3"], bn=bn["bn3"], label="conv3", **mk)
    tail = FusedConv(w["tail"], bn=bn["tail"], label="tail", **mk)
    # the two launches: ft_bottleneck_fwd, then the conv on the full map it wrote
    xv = nchw_to_view(x, dtype, dev)
    y2 = ActView(torch.zeros((N, H, W, C), dtype=dtype, device=dev), C, 0)
    t12 = ActView(torch.zeros((N, H, W, T), dtype=dtype, device=dev), T, 0)
    prog = make_program()
    record_bottleneck(prog, c1, c2, c3, xv, y2, "block", form="patch")
    tail.record(prog, y2, t12)
    prog.resolve_choices()
    assert [n for n, _ in prog.calls][0] == "ft_bottleneck_fwd" and len(prog.calls) == 2
    run_program(prog)
    return dict(x=x, layers=(c1, c2, c3, tail), want_y=want_y, want_t1=want_t1, sep_y=view_to_nchw(y2), sep_t1=view_to_nchw(t12))


def _guarded(shape, poison, dtype, dev):
    """A poisoned buffer with one guard image in front of and one behind the [N, ...] part a launch may write."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), poison, dtype=dtype, device=dev)
    return whole, whole[1:-1]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exit_form_matches_oracle_and_the_two_launches(hip_lib, case):
    name, N, H, W, xcs, xoff, tcs, toff, mode = case
    dev, dtype = torch.device("cuda:0"), torch.float16
    ref = _reference(N, H, W)
    c1, c2, c3, tail = ref["layers"]
    xv = nchw_to_view(ref["x"], dtype, dev, cstride=xcs, coff=xoff)
    if xoff:
        xv.t[..., :xoff] = 7.0          # neighbours of the slice must not leak in
    t1_whole, t1_buf = _guarded((N, H, W, tcs), T_POISON, dtype, dev)
    t1v = ActView(t1_buf, T, toff)
    yv = y_whole = None
    if mode != "none":                  # y into a channel slice as well: 32 pad channels in front
        yh, yw = (H, W) if mode == "full" else (H // 2, W // 2)
        y_whole, y_buf = _guarded((N, yh, yw, C + 32), Y_POISON, dtype, dev)
        yv = ActView(y_buf, C, 32)
    assert bottleneck_exit_fusable(c1, c2, c3, tail, xv, yv, t1v, mode)
    prog = make_program()
    record_bottleneck_exit(prog, c1, c2, c3, tail, xv, yv, t1v, name, mode)
    assert [n for n, _ in prog.calls] == ["ft_bottleneck_exit_fwd"]
    assert len(prog.fused_records) == 1 and prog.fused_records[0][2] == prog.flops
    run_program(prog)

    # ---- t1 ----
    got_t1 = view_to_nchw(t1v)
    scale_t = max(1.0, ref["want_t1"].abs().max().item())
    err = (got_t1 - ref["want_t1"]).abs().max().item()
    diff = (got_t1 - ref["sep_t1"]).abs()
    print(f"{name}: t1 vs oracle {err:.3e} (scale {scale_t:.2f}); vs two launches max {diff.max().item():.3e}, "
          f"{100 * (diff > 0).float().mean().item():.2f} % differ")
    assert err <= 2e-2 * scale_t, f"{name}: t1 vs oracle max abs err {err:.3e} (scale {scale_t:.2f})"
    assert diff.max().item() <= 1e-2 * scale_t, f"{name}: t1 vs the two launches max abs diff {diff.max().item():.3e}"
    assert (diff > 0).float().mean().item() < 0.05, "same roundings as the two launches: only the fp32 summation order may differ"
    # ---- y ----
    if mode != "none":
        got_y = view_to_nchw(yv)
        sel = (lambda t: t) if mode == "full" else (lambda t: t[:, :, ::2, ::2])
        scale_y = max(1.0, ref["want_y"].abs().max().item())
        err_y = (got_y - sel(ref["want_y"])).abs().max().item()
        print(f"{name}: y ({mode}) vs oracle {err_y:.3e} (scale {scale_y:.2f})")
        assert err_y <= 2e-2 * scale_y, f"{name}: y vs oracle max abs err {err_y:.3e} (scale {scale_y:.2f})"
        assert torch.equal(got_y, sel(ref["sep_y"])), "y must hold the bits ft_bottleneck_fwd writes at the same pixels"
        assert torch.all(yv.t[..., :32] == Y_POISON), "channels in front of the y slice were written"
        assert torch.all(y_whole[0] == Y_POISON) and torch.all(y_whole[-1] == Y_POISON), "bytes outside the y view were written"
    # ---- nothing else ----
    assert torch.all(t1v.t[..., :toff] == T_POISON) and torch.all(t1v.t[..., toff + T:] == T_POISON), "pad channels of t1 were written"
    assert torch.all(t1_whole[0] == T_POISON) and torch.all(t1_whole[-1] == T_POISON), "bytes outside the t1 view were written"
    # determinism: same bits on a second run
    t1v.t.fill_(T_POISON)
    run_program(prog)
    assert torch.equal(view_to_nchw(t1v), got_t1)


def test_exit_form_rejects_what_it_does_not_cover(hip_lib):
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def status(N=2, H=16, W=16, dtype=_lib.FT_F16, Cc=C, Pp=P, tail=T, tcs=128, toff=0, xcs=256, xoff=0, mode=_lib.FT_BNK_Y_EVEN):
        d = _lib.BottleneckDesc()
        d.dtype, d.N, d.H, d.W, d.C, d.P = dtype, N, H, W, Cc, Pp
        d.x_cstride, d.x_coff, d.y_cstride, d.y_coff = xcs, xoff, Cc, 0
        return lib.ft_bottleneck_exit_supported(ctypes.byref(d), tail, tcs, toff, mode)
    assert status() == _lib.FT_OK
    assert status(W=15) == _lib.FT_ERR_UNSUPPORTED and status(H=13) == _lib.FT_ERR_UNSUPPORTED          # odd sizes
    assert status(dtype=_lib.FT_F32) == _lib.FT_ERR_UNSUPPORTED
    assert status(xcs=260, xoff=4) == _lib.FT_ERR_UNSUPPORTED and status(tcs=132, toff=4) == _lib.FT_ERR_UNSUPPORTED   # misaligned views
    assert status(tail=64) == _lib.FT_ERR_UNSUPPORTED and status(tail=256, tcs=256) == _lib.FT_ERR_UNSUPPORTED
    assert status(Cc=512, Pp=128, xcs=512) == _lib.FT_ERR_UNSUPPORTED
    assert status(tcs=128, toff=32) == _lib.FT_ERR_INVALID_ARG and status(mode=7) == _lib.FT_ERR_INVALID_ARG
    assert lib.ft_bottleneck_exit_weight_bytes(None, T) == 0
    # the recorder's predicate, and the recorder itself, refuse the same
    c1, c2, c3, tail = _reference(2, 16, 16)["layers"]
    x_odd = ActView(torch.zeros((1, 16, 15, C), dtype=torch.float16, device=dev), C, 0)
    t_odd = ActView(torch.zeros((1, 16, 15, T), dtype=torch.float16, device=dev), T, 0)
    assert not bottleneck_exit_fusable(c1, c2, c3, tail, x_odd, None, t_odd, "none")
    with pytest.raises(FlowtrackHipError):
        record_bottleneck_exit(make_program(), c1, c2, c3, tail, x_odd, None, t_odd, "odd", "none")
    # t1 inside y's buffer (or x's): the launch reads and writes all three at once
    xs = ActView(torch.zeros((1, 16, 16, C), dtype=torch.float16, device=dev), C, 0)
    wide = torch.zeros((1, 16, 16, C + T), dtype=torch.float16, device=dev)
    with pytest.raises(FlowtrackHipError, match="separate"):
        record_bottleneck_exit(make_program(), c1, c2, c3, tail, xs, ActView(wide, C, 0), ActView(wide, T, C), "alias", "full")
    x32 = ActView(torch.zeros((1, 16, 16, C), dtype=torch.float32, device=dev), C, 0)
    t32 = ActView(torch.zeros((1, 16, 16, T), dtype=torch.float32, device=dev), T, 0)
    assert not bottleneck_exit_fusable(c1, c2, c3, tail, x32, None, t32, "none")


def test_plan_with_the_exit_form_matches_the_plan_without(hip_lib, monkeypatch):
    """R50 at 64 x 64, batch 2: the plan with the exit form forced vs the plan that never records it; the heat maps agree to the bar
    tests/test_pose_gpu.py holds fused and plain plans to, and the forced plan has no layer2.0.conv1 launch."""
    monkeypatch.setattr(hip_ops, "benchmark", False)          # the recorder's first option of every other alternative on both sides
    def model(exit_form):
        m = models.deconv("resnet50", num_classes=17, pretrained=False)
        m.load_state_dict(synth.fill_pose_state_dict(m.state_dict(), 1234))
        m = m.cuda().eval()
        m.compute_dtype = torch.float16
        m.fuse_stage_exit = exit_form
        return m
    x = synth.pose_crops(1234 + 7, 2, 64, 64).cuda()
    fused, plain = model("force"), model(False)
    a, b = fused(x).float().cpu(), plain(x).float().cpu()
    pa, pb = fused._last_plan, plain._last_plan
    labels_a, labels_b = [r[0] for r in pa.prog.conv_records], [r[0] for r in pb.prog.conv_records]
    assert "layer2.0.conv1" in labels_b and "layer2.0.conv1" not in labels_a
    assert [n for n, _ in pa.prog.calls].count("ft_bottleneck_exit_fwd") == 1
    assert "ft_bottleneck_exit_fwd" not in [n for n, _ in pb.prog.calls]
    assert len([n for n, _ in pa.prog.calls if hip_ops.is_conv_call(n)]) + 1 == len([n for n, _ in pb.prog.calls if hip_ops.is_conv_call(n)])
    assert abs(pa.prog.flops - pb.prog.flops) <= 1e-9 * pb.prog.flops, "the roofline's FLOPs must not depend on the form"
    rng = (b.max() - b.min()).item()
    err = (a - b).abs().max().item()
    print(f"exit plan vs plain plan: heat maps differ by {err:.3e} (range {rng:.3f})")
    assert err <= 0.02 * rng
    # graph replays (with the benchmark off the first call ran every option of the remaining alternatives, the replays only the first)
    ra, rb = fused(x).float().cpu(), plain(x).float().cpu()
    assert (ra - rb).abs().max().item() <= 0.02 * rng
    assert torch.equal(fused(x).float().cpu(), ra), "two replays of one graph"
    # the full layer1 map does not exist in the exit plan: asking for it must say so, not hand out a partly written buffer
    assert "layer1" in pb.stages and "layer1" not in pa.stages
    with pytest.raises(FlowtrackHipError, match="fuse_stage_exit"):
        pa.stages["layer1"]
