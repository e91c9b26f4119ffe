"""The fragment-stream form of the 64-plane fused blocks (ft_bottleneck_desc.wfrag = 1: weights from L2 straight to registers) against
the LDS-ring form it replaces (FT_BNK_WFRAG=0): same fp16 operands, same fp32 accumulation order, so every output must be BIT-identical.
Oracle parity of the default path is test_bottleneck_gpu.py's / test_bottleneck_exit_gpu.py's business; here only the two forms meet.

Also: the pack entry points without a launch, and a numpy restatement of the stream's fragment order (include/flowtrack_hip.h) that
must take a packed stream apart into exactly the three weight blocks it was built from."""
import ctypes

import numpy as np
import pytest
import torch

from flowtrack.pytorch_amd import _lib, hip_ops, synth
from flowtrack.pytorch_amd.hip_ops import (ActView, FusedConv, FusedShortcutConv, record_bottleneck, record_bottleneck_entry,
                                           record_bottleneck_exit)

# (name, N, H, W): the smallest maps at which the kernel can still go wrong
SHAPES = [
    ("one_patch_8x16", 1, 8, 16),          # every halo pixel lies outside the image
    ("ragged_2x2_12x20", 2, 12, 20),       # 2 x 2 patches, ragged both ways, halo partly inside
    ("interior_rows_24x16", 3, 24, 16),    # a patch row with image rows above and below, image index > 0
    ("tall_patches_18x24", 2, 18, 24),     # width divides by 8 only: the 16 x 8 patch orientation, ragged in y
]
FORMS = ["identity", "projection", "exit_full", "exit_even", "exit_none"]
P, OFF = 64, 32                            # planes; channel offset of every output inside a wider, sentinel-filled buffer
SENTINEL = 3.0


def _bn(seed, name, c):
    return {"weight": synth.uniform(seed, name + "g", (c,), 0.5, 1.5), "bias": synth.normal(seed, name + "b", (c,), 0.1),
            "running_mean": synth.normal(seed, name + "m", (c,), 0.1), "running_var": synth.uniform(seed, name + "v", (c,), 0.5, 1.5),
            "eps": 1e-5}


@pytest.fixture(scope="module")
def layers(hip_lib):
    """One weight set per form, shared by every shape (the stream is cached with c1's packed weights)."""
    dev, dtype, seed = torch.device("cuda:0"), torch.float16, 37
    mk = dict(dtype=dtype, device=dev, act="relu")
    C = 4 * P
    he = lambda fan: (2.0 / fan) ** 0.5
    out = {}
    for form, cin in (("identity", C), ("projection", P), ("exit", C)):
        c1 = FusedConv(synth.normal(seed, form + ".w1", (P, cin, 1, 1), std=he(cin)), bn=_bn(seed, form + ".bn1", P), **mk)
        c2 = FusedConv(synth.normal(seed, form + ".w2", (P, P, 3, 3), std=he(9 * P)), pad=1, bn=_bn(seed, form + ".bn2", P), **mk)
        if form == "projection":
            c3 = FusedShortcutConv(synth.normal(seed, form + ".w3", (C, P, 1, 1), std=he(P)), _bn(seed, form + ".bn3", C),
                                   synth.normal(seed, form + ".wd", (C, P, 1, 1), std=he(P)), _bn(seed, form + ".bnd", C), 1,
                                   dtype=dtype, device=dev, act="relu")
        else:
            c3 = FusedConv(synth.normal(seed, form + ".w3", (C, P, 1, 1), std=he(P)), bn=_bn(seed, form + ".bn3", C), **mk)
        out[form] = (c1, c2, c3)
    out["tail"] = FusedConv(synth.normal(seed, "tail.w", (2 * P, C, 1, 1), std=he(C)), bn=_bn(seed, "tail.bn", 2 * P), **mk)
    return out


def _record_and_run(layers, form, x, N, H, W):
    """Records the block into a fresh program, runs it; returns (program, [output buffers])."""
    dev, dtype, C = x.t.device, x.t.dtype, 4 * P
    full = lambda n, h, w, c: ActView(torch.full((n, h, w, c + OFF), SENTINEL, dtype=dtype, device=dev), c, OFF)
    prog = hip_ops.Program(torch.cuda.Stream())
    if form == "identity":
        outs = [full(N, H, W, C)]
        record_bottleneck(prog, *layers["identity"], x, outs[0], form, form="patch")
    elif form == "projection":
        outs = [full(N, H, W, C)]
        record_bottleneck_entry(prog, *layers["projection"], x, outs[0], form)
    else:
        mode = form.split("_")[1]
        y = {"full": lambda: full(N, H, W, C), "even": lambda: full(N, H // 2, W // 2, C), "none": lambda: None}[mode]()
        t1 = full(N, H, W, 2 * P)
        outs = [t1] + ([y] if y is not None else [])
        record_bottleneck_exit(prog, *layers["exit"], layers["tail"], x, y, t1, form, mode)
    torch.cuda.synchronize()
    prog.run_eager()
    prog.stream.synchronize()
    return prog, outs


def _stream_env(monkeypatch, form):
    """The environment under which the recorder takes the stream form: the default for the identity and projection blocks; the
    exit form records the ring by default (it lost its A/B) and has the stream behind FT_BNK_WFRAG=1."""
    if form.startswith("exit"):
        monkeypatch.setenv("FT_BNK_WFRAG", "1")
    else:
        monkeypatch.delenv("FT_BNK_WFRAG", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_fragment_stream_form_is_bit_identical_to_the_ring_form(layers, monkeypatch, shape, form):
    name, N, H, W = shape
    dev, dtype = torch.device("cuda:0"), torch.float16
    cin = P if form == "projection" else 4 * P
    x = ActView(synth.normal(41, name + form, (N, H, W, cin)).to(dev).to(dtype), cin, 0)

    monkeypatch.setenv("FT_BNK_WFRAG", "0")
    prog_ring, ring = _record_and_run(layers, form, x, N, H, W)
    _stream_env(monkeypatch, form)
    prog_frag, frag = _record_and_run(layers, form, x, N, H, W)

    # the two programs are the two forms of the same entry point
    (n0, a0), (n1, a1) = prog_ring.calls[-1], prog_frag.calls[-1]
    assert n0 == n1 == ("ft_bottleneck_fwd" if not form.startswith("exit") else "ft_bottleneck_exit_fwd")
    assert a0[0]._obj.wfrag == 0 and a0[3] is not None and a0[4] is not None
    assert a1[0]._obj.wfrag == 1 and a1[3] is None and a1[4] is None

    for r, f in zip(ring, frag):
        assert torch.isfinite(r.t.float()).all() and r.t[..., OFF:].float().abs().max().item() > 0.1, "the ring form wrote nothing"
        assert torch.equal(r.t, f.t), f"{name} {form}: {(r.t != f.t).sum().item()} of {r.t.numel()} values differ"
        assert torch.all(f.t[..., :OFF] == SENTINEL), "channels outside the output slice were written"
    # a second run of the new form: same bits into buffers that held something else
    first = [f.t.clone() for f in frag]
    for f in frag:
        f.t[..., OFF:] = -5.0
    torch.cuda.synchronize()
    prog_frag.run_eager()
    prog_frag.stream.synchronize()
    for a, f in zip(first, frag):
        assert torch.equal(a, f.t)


# ---- the stream's layout, restated in numpy ------------------------------------------------------------------------------------
def frag_sources(nch, proj):
    """For every 16-byte unit of the stream, in order: (block 0 / 1 / 2 = W1 / W2 / W3, row, first k).  Blocks are row-major fp16:
    W1 [64][64 nch], W2 [64][576], W3 [256][64] (projection: [256][128] = W3' | Wd')."""
    units = []

    def frag(block, row0, k0):
        for lane in range(64):
            units.append((block, row0 + lane % 32, k0 + 8 * (lane // 32)))
    for c in range(nch):
        for tile in range(2):
            for s in range(4):
                frag(0, 32 * tile, 64 * c + 16 * s)
    for tap in range(9):
        for tile in range(2):
            for s in range(4):
                frag(1, 32 * tile, 64 * tap + 16 * s)
    for q in range(4):
        for tile in range(2):
            for s in range(8 if proj else 4):
                frag(2, 64 * q + 32 * tile, 16 * s)
    return units


def unpack_stream(stream_u16, nch, proj):
    """stream (uint16 view of the bytes) -> [W1, W2, W3] and how often every element was written."""
    shapes = [(64, 64 * nch), (64, 576), (256, 128 if proj else 64)]
    blocks = [np.zeros(s, np.uint16) for s in shapes]
    hits = [np.zeros(s, np.int32) for s in shapes]
    units = frag_sources(nch, proj)
    assert stream_u16.size == 8 * len(units)
    for i, (b, r, k) in enumerate(units):
        blocks[b][r, k:k + 8] = stream_u16[8 * i:8 * i + 8]
        hits[b][r, k:k + 8] += 1
    return blocks, hits


@pytest.mark.parametrize("nch,proj,nbytes", [(4, False, 139264), (1, True, 147456)])
def test_fragment_order_covers_every_weight_once(nch, proj, nbytes):
    """No GPU: the restated order has the documented size and touches every element of the three blocks exactly once."""
    units = frag_sources(nch, proj)
    assert 16 * len(units) == nbytes
    rng = np.random.default_rng(5)
    shapes = [(64, 64 * nch), (64, 576), (256, 128 if proj else 64)]
    src = [rng.integers(0, 65536, s).astype(np.uint16) for s in shapes]
    stream = np.concatenate([src[b][r, k:k + 8] for b, r, k in units])
    blocks, hits = unpack_stream(stream, nch, proj)
    assert all((h == 1).all() for h in hits)
    assert all((a == b).all() for a, b in zip(blocks, src))


def _desc(**kw):
    d = _lib.BottleneckDesc()
    base = dict(dtype=0, N=2, H=12, W=20, C=256, P=64, x_cstride=256, x_coff=0, y_cstride=256, y_coff=0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_frag_entry_points_check_their_arguments(hip_lib):
    """No launch happens (no GPU needed): sizes, NULL operands, wfrag = 1 with a second weight pointer."""
    ok, invalid, unsupported = 0, 1, 2
    nbytes = lambda **kw: hip_lib.ft_bottleneck_frag_bytes(ctypes.byref(_desc(**kw)))
    assert nbytes() == 1024 * (8 * 4 + 72 + 32) == 139264
    assert nbytes(C=64, x_cstride=64, projection=1) == 1024 * (8 + 72 + 64) == 147456
    assert nbytes(C=64, x_cstride=64, y_cstride=64, head_only=1) == 0 and nbytes(P=128) == 0 and hip_lib.ft_bottleneck_frag_bytes(None) == 0
    one = ctypes.c_void_p(16)            # never dereferenced: every call below returns before a launch
    pack = lambda d, *a: hip_lib.ft_bottleneck_frag_pack(ctypes.byref(d), *a, None)
    assert pack(_desc(), None, one, one, one) == invalid and pack(_desc(), one, None, one, one) == invalid
    assert pack(_desc(), one, one, None, one) == invalid and pack(_desc(), one, one, one, None) == invalid
    assert pack(_desc(C=64, x_cstride=64, y_cstride=64, head_only=1), one, one, one, one) == unsupported
    assert hip_lib.ft_bottleneck_frag_pack(None, one, one, one, one, None) == invalid
    fwd = lambda d, w1, w2, w3: hip_lib.ft_bottleneck_fwd(ctypes.byref(d), one, w1, w2, w3, one, one, None)
    assert hip_lib.ft_bottleneck_supported(ctypes.byref(_desc(wfrag=1))) == ok
    assert fwd(_desc(wfrag=1), one, one, None) == invalid and fwd(_desc(wfrag=1), one, None, one) == invalid    # w1 is the whole stream
    assert fwd(_desc(wfrag=1), None, None, None) == invalid
    assert fwd(_desc(wfrag=0), one, None, one) == invalid and fwd(_desc(wfrag=0), one, one, None) == invalid
    assert hip_lib.ft_bottleneck_supported(ctypes.byref(_desc(wfrag=2))) == invalid
    assert hip_lib.ft_bottleneck_supported(ctypes.byref(_desc(C=64, x_cstride=64, y_cstride=64, head_only=1, wfrag=1))) == unsupported
    exit_fwd = lambda d, w2, w3: hip_lib.ft_bottleneck_exit_fwd(ctypes.byref(d), one, one, w2, w3, one, one, 0, 128, one, one, one, one, 128, 0, None)
    assert exit_fwd(_desc(wfrag=1), one, None) == invalid and exit_fwd(_desc(wfrag=1), None, one) == invalid
    assert exit_fwd(_desc(wfrag=0), None, one) == invalid


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["identity", "projection", "exit_even"])
def test_packed_stream_unpacks_to_the_three_weight_blocks(layers, monkeypatch, form):
    """ft_bottleneck_frag_pack's output, taken apart by the numpy restatement, is W1, W2 and W3 as the ring form gets them."""
    _stream_env(monkeypatch, form)
    N, H, W = 1, 8, 16
    cin = P if form == "projection" else 4 * P
    x = ActView(torch.zeros((N, H, W, cin), dtype=torch.float16, device="cuda:0"), cin, 0)
    _record_and_run(layers, form, x, N, H, W)
    c1 = layers[form.split("_")[0]][0]
    cached = [v for k, v in c1._packed.items() if k[0] == "bnk_frag"]
    assert len(cached) == 1
    stream, w1, w2, w3 = cached[0]
    proj, nch = form == "projection", cin // 64
    assert stream.numel() == (147456 if proj else 139264)
    blocks, hits = unpack_stream(stream.cpu().numpy().view(np.uint16), nch, proj)
    assert all((h == 1).all() for h in hits)
    for got, w in zip(blocks, (w1, w2, w3)):
        want = w.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).reshape(got.shape)
        assert (got == want).all()
