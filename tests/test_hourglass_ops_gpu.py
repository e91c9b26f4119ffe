"""ft_hourglass_down_fwd and ft_hourglass_up_fwd alone, through the C ABI (include/flowtrack_hip.h), fp16 and fp32.

down: the pooled map bit for bit against numpy's max (an odd last row / column holds a huge value, so a pool that reads it shows);
a_full / a_pool bit for bit against ft_scale_shift_act_nhwc_fwd run on x and on the STORED pool; an integer-grid case that is exact
in any arithmetic against numpy; every subset of the three outputs; channel windows inside wider buffers with sentinels around
them; past the grid's caps (more than 64 x 256 items in a row, more than 65535 images); refusals.
up: the sum against the float64 reference within the derived bound (hourglass_ref.up_bound); a_sum bit for bit against
ft_scale_shift_act_nhwc_fwd on the stored sum; equal sizes give dtype(skip + low) exactly; in place equals out of place."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import hourglass_ref
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import FT_ERR_INVALID_ARG, FT_F16, check

pytestmark = pytest.mark.gpu
SENTINEL = 99.0
HUGE = 60000.0                                # fits fp16; no random value comes near it
GUARD = 8                                     # elements around a buffer: 16 or 32 bytes, so the 16-byte alignment is kept
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
FT_ACT_RELU = 1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _group(dtype):
    return 8 if dtype == torch.float16 else 4


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


class _Buf:
    """An NHWC buffer [N,H,W,cstride] full of sentinels between two guards, on the GPU; the channel window is [coff, coff + C)."""

    def __init__(self, N, H, W, C, cstride, coff, dtype, fill=None):
        self.shape, self.C, self.cstride, self.coff = (N, H, W, cstride), C, cstride, coff
        n = N * H * W * cstride
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.flat[GUARD:GUARD + n].view(N, H, W, cstride)
        assert self.view.data_ptr() % 16 == 0
        if fill is not None:
            self.view[..., coff:coff + C] = fill.to(dtype).cuda()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def window(self):
        """The channel window on the CPU, after checking that nothing around it was written."""
        flat = self.flat.cpu()
        n = flat.numel() - 2 * GUARD
        win = flat[GUARD:GUARD + n].view(self.shape)
        outside = torch.ones(self.cstride, dtype=torch.bool)
        outside[self.coff:self.coff + self.C] = False
        assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + n:] == SENTINEL).all()), "wrote outside the buffer"
        assert bool((win[..., outside] == SENTINEL).all()), "wrote outside the channel window [coff, coff + C)"
        return win[..., self.coff:self.coff + self.C].contiguous()

    def untouched(self):
        return bool((self.flat.cpu() == SENTINEL).all())


def _ssa(hip_lib, x, scale, shift):
    """ft_scale_shift_act_nhwc_fwd (ReLU) on a dense NHWC CPU tensor -> CPU tensor of the same dtype."""
    xd = x.contiguous().cuda()
    y = torch.empty_like(xd)
    C = x.shape[-1]
    s, b = scale.float().cuda().contiguous(), shift.float().cuda().contiguous()
    check(hip_lib.ft_scale_shift_act_nhwc_fwd(xd.data_ptr(), y.data_ptr(), _lib.dtype_code(x.dtype), ctypes.c_longlong(x.numel() // C), C, C, 0, C, 0,
                                              s.data_ptr(), b.data_ptr(), FT_ACT_RELU, ctypes.c_float(0.0), _stream()), "ft_scale_shift_act_nhwc_fwd")
    torch.cuda.synchronize()
    return y.cpu()


def _tables(name, C):
    s = synth.uniform(11, "hg.ops.scale." + name, (C,), 0.5, 1.5) * (1 - 2 * (torch.arange(C) % 3 == 1).float())      # both signs
    return s, synth.normal(11, "hg.ops.shift." + name, (C,), std=0.5)


def _down_input(name, N, H, W, C, dtype):
    x = synth.normal(11, "hg.ops.down." + name, (N, H, W, C)).to(dtype)
    if H % 2:
        x[:, H - 1] = HUGE
    if W % 2:
        x[:, :, W - 1] = HUGE
    return x


def _down(hip_lib, x, dtype, tabs_pool, tabs_full, outs=("pool", "a_pool", "a_full"), cstride=None, coff=0):
    """x: [N,H,W,C] CPU tensor of `dtype`.  Runs the kernel with the outputs named in `outs` (the others NULL, their buffers
    allocated all the same) and returns {name: window on the CPU}; every buffer is checked for writes outside its window, a buffer
    that was not passed for any write at all, and x for being left alone."""
    N, H, W, C = x.shape
    G = _group(dtype)
    cstride = (coff + C + G - 1) // G * G if cstride is None else cstride
    xb = _Buf(N, H, W, C, cstride, coff, dtype, fill=x)
    bufs = {"pool": _Buf(N, H // 2, W // 2, C, cstride, coff, dtype), "a_pool": _Buf(N, H // 2, W // 2, C, cstride, coff, dtype),
            "a_full": _Buf(N, H, W, C, cstride, coff, dtype)}
    tp = [t.float().cuda().contiguous() for t in tabs_pool]
    tf = [t.float().cuda().contiguous() for t in tabs_full]

    def arg(name):
        return (bufs[name].ptr if name in outs else None, cstride, coff)
    check(hip_lib.ft_hourglass_down_fwd(xb.ptr, _lib.dtype_code(dtype), N, H, W, C, cstride, coff, *arg("pool"), *arg("a_pool"), tp[0].data_ptr(),
                                        tp[1].data_ptr(), *arg("a_full"), tf[0].data_ptr(), tf[1].data_ptr(), _stream()), "ft_hourglass_down_fwd")
    torch.cuda.synchronize()
    assert torch.equal(_bits(xb.window()), _bits(x)), "the input changed"
    for name, b in bufs.items():
        if name not in outs:
            assert b.untouched(), f"{name} was passed as NULL and its buffer was written"
    return {name: bufs[name].window() for name in outs}


def _check_down(hip_lib, name, N, H, W, C, dtype, outs=("pool", "a_pool", "a_full"), **view):
    x = _down_input(name, N, H, W, C, dtype)
    tp, tf = _tables(name + ".pool", C), _tables(name + ".full", C)
    got = _down(hip_lib, x, dtype, tp, tf, outs, **view)
    want_pool = torch.from_numpy(hourglass_ref.down_ref(x.numpy()))
    assert not bool((want_pool == HUGE).any())
    if "pool" in outs:
        assert torch.equal(_bits(got["pool"]), _bits(want_pool)), f"{name}: pool differs from numpy's max"
    if "a_pool" in outs:
        assert torch.equal(_bits(got["a_pool"]), _bits(_ssa(hip_lib, want_pool, *tp))), f"{name}: a_pool differs from scale_shift_act(pool)"
    if "a_full" in outs:
        assert torch.equal(_bits(got["a_full"]), _bits(_ssa(hip_lib, x, *tf))), f"{name}: a_full differs from scale_shift_act(x)"


DOWN_SHAPES = [("one_cell", 1, 2, 2, 8), ("odd_sides_tail", 2, 5, 7, 20), ("odd_rows_c256", 1, 3, 2, 256), ("c256", 3, 16, 12, 256),
               ("level_top", 2, 64, 48, 256),
               ("past_row_cap", 1, 2, 1042, 256),       # 521 cells x 32 / 64 groups: more than the 64 x 256 items one pass of a row covers
               ("past_image_cap", 65540, 2, 2, 8)]      # more images than the grid's y extent


@DTYPES
@pytest.mark.parametrize("case", DOWN_SHAPES, ids=[c[0] for c in DOWN_SHAPES])
def test_down_matches_pool_and_scale_shift_act(hip_lib, case, dtype):
    _check_down(hip_lib, *case, dtype)


@DTYPES
def test_down_sliced_view(hip_lib, dtype):
    _check_down(hip_lib, "sliced", 2, 6, 5, 24, dtype, cstride=40, coff=8)


@DTYPES
@pytest.mark.parametrize("outs", [c for r in (1, 2, 3) for c in itertools.combinations(("pool", "a_pool", "a_full"), r)], ids="+".join)
def test_down_output_subsets(hip_lib, outs, dtype):
    _check_down(hip_lib, "subsets", 2, 5, 7, 20, dtype, outs=outs)


@DTYPES
def test_down_integer_grid_exact(hip_lib, dtype):
    """Integer x in [-64, 64], scales in {+-0.5, +-1, +-2}, shifts multiples of 0.5: every product and sum is exact in fp32 and in
    fp16, so all three outputs equal numpy's, bit for bit, whatever the arithmetic's order or fusion."""
    N, H, W, C = 2, 7, 6, 20
    x = torch.from_numpy(np.floor(synth.uniform01(13, "hg.ops.grid.x", (N, H, W, C)) * 129.0) - 64.0).to(dtype)

    def tables(tag):
        s = np.array([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[(synth.uniform01(13, "hg.ops.grid.s" + tag, (C,)) * 6).astype(np.int64)]
        b = np.floor(synth.uniform01(13, "hg.ops.grid.b" + tag, (C,)) * 65.0 - 32.0) * 0.5
        return torch.from_numpy(s).float(), torch.from_numpy(b).float()
    tp, tf = tables("p"), tables("f")
    got = _down(hip_lib, x, dtype, tp, tf)
    npdt = np.float16 if dtype == torch.float16 else np.float32
    pool = hourglass_ref.down_ref(x.numpy())
    assert torch.equal(_bits(got["pool"]), _bits(torch.from_numpy(pool)))
    assert torch.equal(_bits(got["a_pool"]), _bits(torch.from_numpy(hourglass_ref.affine_relu_exact(pool, tp[0].numpy(), tp[1].numpy(), npdt))))
    assert torch.equal(_bits(got["a_full"]), _bits(torch.from_numpy(hourglass_ref.affine_relu_exact(x.numpy(), tf[0].numpy(), tf[1].numpy(), npdt))))


def test_down_refusals(hip_lib):
    N, H, W, C = 1, 4, 4, 16
    x = torch.zeros((N, H, W, C), dtype=torch.float16, device="cuda")
    pool, a_pool = (torch.zeros((N, 2, 2, C), dtype=torch.float16, device="cuda") for _ in range(2))
    a_full = torch.zeros_like(x)
    s = torch.ones(C, device="cuda")

    def call(x=x.data_ptr(), dtype=FT_F16, N=N, H=H, W=W, C=C, xs=C, xo=0, pool=pool.data_ptr(), ps=C, po=0, a_pool=a_pool.data_ptr(), aps=C, apo=0,
             sp=s.data_ptr(), bp=s.data_ptr(), a_full=a_full.data_ptr(), afs=C, afo=0, sf=s.data_ptr(), bf=s.data_ptr()):
        return hip_lib.ft_hourglass_down_fwd(x, dtype, N, H, W, C, xs, xo, pool, ps, po, a_pool, aps, apo, sp, bp, a_full, afs, afo, sf, bf, _stream())
    assert call() == 0
    bad = [dict(x=None), dict(pool=None, a_pool=None, a_full=None), dict(N=0), dict(H=0), dict(W=0), dict(C=0), dict(dtype=7),
           dict(H=1), dict(W=1), dict(H=1, pool=None), dict(sp=None), dict(bp=None), dict(sf=None), dict(bf=None),
           dict(xo=4), dict(xs=20), dict(po=4), dict(aps=20), dict(afo=-8), dict(xs=8), dict(x=x.data_ptr() + 2), dict(pool=pool.data_ptr() + 8),
           dict(a_full=x.data_ptr()), dict(a_pool=pool.data_ptr()), dict(pool=a_full.data_ptr()), dict(sf=s.data_ptr() + 2)]
    for kw in bad:
        assert call(**kw) == FT_ERR_INVALID_ARG, kw
    assert call(H=1, pool=None, a_pool=None) == 0          # a_full alone has no lower bound on the sides
    # disjoint channel windows of ONE buffer are no overlap: pool in [0, 16), a_pool in [16, 32) of a 32-channel buffer
    both = torch.zeros((N, 2, 2, 32), dtype=torch.float16, device="cuda")
    assert call(pool=both.data_ptr(), ps=32, po=0, a_pool=both.data_ptr(), aps=32, apo=16) == 0
    assert call(pool=both.data_ptr(), ps=32, po=0, a_pool=both.data_ptr(), aps=32, apo=8) == FT_ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---- the way up ----------------------------------------------------------------------------------------------------------------------
def _up(hip_lib, skip, low, dtype, tabs=None, in_place=False, cstride=None, coff=0):
    """skip [N,H,W,C], low [N,hl,wl,C]: CPU tensors of `dtype` -> (sum window, a_sum window or None) on the CPU."""
    N, H, W, C = skip.shape
    G = _group(dtype)
    cstride = (coff + C + G - 1) // G * G if cstride is None else cstride
    kb = _Buf(N, H, W, C, cstride, coff, dtype, fill=skip)
    lb = _Buf(N, low.shape[1], low.shape[2], C, cstride, coff, dtype, fill=low)
    sb = kb if in_place else _Buf(N, H, W, C, cstride, coff, dtype)
    ab = _Buf(N, H, W, C, cstride, coff, dtype)
    t = [v.float().cuda().contiguous() for v in tabs] if tabs is not None else None
    check(hip_lib.ft_hourglass_up_fwd(kb.ptr, lb.ptr, _lib.dtype_code(dtype), N, C, H, W, low.shape[1], low.shape[2], cstride, coff, cstride, coff,
                                      sb.ptr, cstride, coff, ab.ptr if t else None, cstride, coff, t[0].data_ptr() if t else None,
                                      t[1].data_ptr() if t else None, _stream()), "ft_hourglass_up_fwd")
    torch.cuda.synchronize()
    assert torch.equal(_bits(lb.window()), _bits(low)), "low changed"
    if not in_place:
        assert torch.equal(_bits(kb.window()), _bits(skip)), "skip changed"
    if t is None:
        assert ab.untouched()
    return sb.window(), (ab.window() if t else None)


#: (name, N, C, hl, wl, H, W)
UP_CASES = [("ratio0", 1, 8, 1, 1, 2, 2), ("ratio0_3x2", 2, 20, 1, 1, 3, 2), ("2x3_5x6", 2, 20, 2, 3, 5, 6), ("3x2_6x5", 1, 256, 3, 2, 6, 5),
            ("8x6_16x12", 3, 256, 8, 6, 16, 12), ("c8", 2, 8, 3, 2, 6, 5), ("level_top", 2, 256, 32, 24, 64, 48)]


def _up_data(name, N, C, hl, wl, H, W, dtype):
    return (synth.normal(12, "hg.ops.up.skip." + name, (N, H, W, C)).to(dtype), synth.normal(12, "hg.ops.up.low." + name, (N, hl, wl, C)).to(dtype))


def _check_up(hip_lib, case, dtype, **view):
    name, N, C = case[0], case[1], case[2]
    skip, low = _up_data(*case, dtype)
    tabs = _tables("up." + name, C)
    got, a = _up(hip_lib, skip, low, dtype, tabs, **view)
    want, mag = hourglass_ref.up_ref(skip, low)
    bound = hourglass_ref.up_bound(want, mag, fp16=dtype == torch.float16)
    ratio = ((got.double() - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"up {name} {dtype}: worst error / derived bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the derived bound"
    assert torch.equal(_bits(a), _bits(_ssa(hip_lib, got, *tabs))), f"{name}: a_sum differs from scale_shift_act(sum as stored)"
    # the same sum without a_sum, and in place: bit for bit
    alone, none = _up(hip_lib, skip, low, dtype, None, **view)
    assert none is None and torch.equal(_bits(alone), _bits(got))
    inpl, a2 = _up(hip_lib, skip, low, dtype, tabs, in_place=True, **view)
    assert torch.equal(_bits(inpl), _bits(got)) and torch.equal(_bits(a2), _bits(a))


@DTYPES
@pytest.mark.parametrize("case", UP_CASES, ids=[c[0] for c in UP_CASES])
def test_up_sum_within_bound_and_activation_bits(hip_lib, case, dtype):
    _check_up(hip_lib, case, dtype)


@DTYPES
def test_up_sliced_view(hip_lib, dtype):
    _check_up(hip_lib, ("sliced", 2, 24, 2, 3, 5, 6), dtype, cstride=40, coff=8)


@DTYPES
def test_up_equal_sizes_is_plain_add(hip_lib, dtype):
    """hl, wl == H, W: every weight is 0 or 1, the sum is dtype(skip + low) exactly."""
    skip, low = _up_data("same", 2, 20, 5, 6, 5, 6, dtype)
    got, _ = _up(hip_lib, skip, low, dtype)
    assert torch.equal(_bits(got), _bits((skip.float() + low.float()).to(dtype)))      # (fp16 + fp16 is exact in fp32: one rounding)


def test_up_refusals(hip_lib):
    N, C, H, W, hl, wl = 1, 16, 4, 4, 2, 2
    skip = torch.zeros((N, H, W, C), dtype=torch.float16, device="cuda")
    out, a = torch.zeros_like(skip), torch.zeros_like(skip)
    low = torch.zeros((N, hl, wl, C), dtype=torch.float16, device="cuda")
    s = torch.ones(C, device="cuda")

    def call(skip=skip.data_ptr(), low=low.data_ptr(), dtype=FT_F16, N=N, C=C, H=H, W=W, hl=hl, wl=wl, ks=C, ko=0, ls=C, lo=0, out=out.data_ptr(), ss=C,
             so=0, a=a.data_ptr(), as_=C, ao=0, sc=s.data_ptr(), sh=s.data_ptr()):
        return hip_lib.ft_hourglass_up_fwd(skip, low, dtype, N, C, H, W, hl, wl, ks, ko, ls, lo, out, ss, so, a, as_, ao, sc, sh, _stream())
    assert call() == 0 and call(out=skip.data_ptr()) == 0 and call(a=None, sc=None, sh=None) == 0
    bad = [dict(skip=None), dict(low=None), dict(out=None), dict(N=0), dict(C=0), dict(H=0), dict(W=0), dict(hl=0), dict(wl=0), dict(dtype=3),
           dict(sc=None), dict(sh=None), dict(ko=4), dict(ls=20), dict(so=4), dict(as_=8), dict(skip=skip.data_ptr() + 2),
           dict(out=low.data_ptr()), dict(out=skip.data_ptr() + 32), dict(a=skip.data_ptr()), dict(a=out.data_ptr()), dict(a=low.data_ptr())]
    for kw in bad:
        assert call(**kw) == FT_ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
