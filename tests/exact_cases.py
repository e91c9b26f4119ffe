"""Integer-valued data, power-of-two BatchNorms and float64 references for the bit-exact tests of the conv and fused-bottleneck kernels
(test_exact_cases_cpu.py checks the cases themselves, test_conv_exact_gpu.py / test_bottleneck_exact_gpu.py run the kernels).

With small integers as inputs, weights, shifts and residuals every fp16 x fp16 product is exact, every fp32 partial sum is exact in
any summation order, scales of +-1 / +-2 / +-0.5 survive the fp32 scale table and the folding into fp16 weights unchanged, and every
value a kernel stores in fp16 is representable (integers up to 2048, half-integers up to 1024): the kernel's output must EQUAL the
float64 reference element for element, whatever tile, K split, fold setting or form computed it.

A reference is a `Chain` of `Layer`s in float64, so that the CPU test can tamper with one product of one layer (drop it / count it
twice) and see the result change."""
import functools

import torch
import torch.nn.functional as F

from flowtrack.pytorch_amd import synth

SEED = 47
SLOPE = 0.5          # LeakyReLU slope of the leaky cases: negative outputs stay representable, and 0.5 still takes the leaky path


# ---- data --------------------------------------------------------------------------------------------------------------------------
def ints(seed, name, shape, p, amax):
    """float64 tensor: zero with probability 1 - p, else +- an integer in 1..amax; built on synth.uniform (same on every machine)."""
    u = synth.uniform(seed, name + ".u", shape).double()
    v = synth.uniform(seed, name + ".v", shape).double()
    s = synth.uniform(seed, name + ".s", shape).double()
    mag = torch.clamp(torch.floor(v * amax), max=amax - 1) + 1.0
    return torch.where(u < p, torch.where(s < 0.5, -mag, mag), torch.zeros_like(mag))


def cover_weights(w, out_dim=0):
    """Give every (tap, input channel) column and every output channel of a sparse weight tensor a non-zero entry (+-1)."""
    m = w.movedim(out_dim, 0)
    flat = m.reshape(m.shape[0], -1).clone()
    cout, K = flat.shape
    cols = (flat.abs().sum(0) == 0).nonzero().flatten()
    flat[cols % cout, cols] = torch.where(cols % 2 == 0, 1.0, -1.0).double()
    rows = (flat.abs().sum(1) == 0).nonzero().flatten()
    flat[rows, (rows * 7) % K] = 1.0
    return flat.reshape(m.shape).movedim(0, out_dim).contiguous()


def cover_input(x):
    """Give every channel of every image a non-zero pixel."""
    x = x.clone()
    N, C, H, W = x.shape
    n, c = (x.abs().sum((2, 3)) == 0).nonzero(as_tuple=True)
    pix = (n * 5 + c * 3) % (H * W)
    x[n, c, pix // W, pix % W] = torch.where(c % 2 == 0, 1.0, -1.0).double()
    return x


def int_input(name, shape, p=0.5, amax=2):
    return cover_input(ints(SEED, name, shape, p, amax))


def int_weights(name, shape, p, out_dim=0, amax=1):
    return cover_weights(ints(SEED, name, shape, min(p, 0.5), amax), out_dim)


POW2 = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)


def pow2_bn(name, c, scales=POW2, amax=8):
    """BatchNorm whose folded scale is exactly one of `scales` (running_var 1, eps 0) and whose folded shift is a (half-)integer."""
    u = synth.uniform(SEED, name + ".g", (c,))
    g = torch.tensor(scales, dtype=torch.float32)[torch.clamp((u * len(scales)).long(), max=len(scales) - 1)]
    return {"weight": g, "bias": ints(SEED, name + ".b", (c,), 1.0, amax).float(), "running_mean": ints(SEED, name + ".m", (c,), 0.75, amax).float(),
            "running_var": torch.ones(c), "eps": 0.0}


def fold64(cout, bias, bn):
    """The layer's (scale, shift) in float64, restated from the definition of eval-mode BatchNorm (hip_ops.fold_scale_shift)."""
    scale, shift = torch.ones(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
    if bn is not None:
        scale = bn["weight"].double() / torch.sqrt(bn["running_var"].double() + bn["eps"])
        shift = bn["bias"].double() - bn["running_mean"].double() * scale
    if bias is not None:
        shift = shift + bias.double() * scale
    return scale, shift


# ---- float64 reference chains --------------------------------------------------------------------------------------------------------
def conv64(x, w, stride=1, pad=0):
    """F.conv2d in float64; a 1x1 conv as one matrix product (much faster on the large maps)."""
    if w.shape[2] == 1 and w.shape[3] == 1 and pad == 0:
        xs = x[:, :, ::stride, ::stride]
        return torch.matmul(w[:, :, 0, 0], xs.reshape(xs.shape[0], xs.shape[1], -1)).view(xs.shape[0], w.shape[0], xs.shape[2], xs.shape[3])
    return F.conv2d(x, w, stride=stride, padding=pad)


class Branch:
    def __init__(self, src, w, stride=1, pad=0, transposed=False, scale=None):
        self.src, self.w, self.stride, self.pad, self.transposed, self.scale = src, w, stride, pad, transposed, scale

    def conv(self, x):
        if self.transposed:
            return F.conv_transpose2d(x, self.w, stride=self.stride, padding=self.pad)
        return conv64(x, self.w, self.stride, self.pad)


class Layer:
    """out = post(act(sum_b conv_b(T[src_b]) * scale_b + shift + T[res]))."""

    def __init__(self, out, branches, shift=None, act=None, slope=SLOPE, res=None, post=None):
        self.out, self.branches, self.shift, self.act, self.slope, self.res, self.post = out, branches, shift, act, slope, res, post

    def pre(self, T):
        acc = None
        for b in self.branches:
            c = b.conv(T[b.src])
            if b.scale is not None:
                c = c * b.scale.view(1, -1, 1, 1)
            acc = c if acc is None else acc + c
        return acc if self.shift is None else acc + self.shift.view(1, -1, 1, 1)

    def finish(self, v, r=None):
        """Elementwise part of the epilogue (v: pre, whole or one element; r: the residual at the same place)."""
        if r is not None:
            v = v + r
        if self.act == "relu":
            v = torch.clamp(v, min=0.0)
        elif self.act == "leaky":
            v = torch.where(v > 0, v, v * self.slope)
        return v

    def run(self, T, pre=None):
        v = self.finish(self.pre(T) if pre is None else pre, T[self.res] if self.res else None)
        return v if self.post is None else self.post(v)


class Chain:
    def __init__(self, name, inputs, layers, outputs, stored=(), act=None, meta=None):
        """inputs: name -> float64 tensor; outputs: names of the tensors a launch writes; stored: further tensors a kernel keeps in
        fp16 on the way (t1, t2, the tail's input)."""
        self.name, self.inputs, self.layers, self.outputs, self.stored = name, inputs, layers, tuple(outputs), tuple(stored)
        self.meta = meta or {}
        self._T = None

    @property
    def T(self):
        if self._T is None:
            T = dict(self.inputs)
            for L in self.layers:
                T["pre:" + L.out] = L.pre(T)
                T[L.out] = L.run(T, T["pre:" + L.out])
            self._T = T
        return self._T

    def __getitem__(self, k):
        return self.T[k]

    def tampered(self, li, idx, delta):
        """The outputs with `delta` added to ONE element `idx` of layer li's sum (a product dropped or counted twice).  Returns a list
        of (reference part, tampered part) pairs that cover every place the change can reach."""
        T, L = self.T, self.layers[li]
        if li == len(self.layers) - 1 and L.post is None:
            r = T[L.res][idx] if L.res else None
            return [(T[L.out][idx], L.finish(T["pre:" + L.out][idx] + delta, r))]
        pre = T["pre:" + L.out].clone()
        pre[idx] += delta
        N = dict(T)
        N[L.out] = L.run(N, pre)
        for M in self.layers[li + 1:]:
            N[M.out] = M.run(N)
        return [(T[o], N[o]) for o in self.outputs]


def _epilogue(name, cout, norm, scales=POW2):
    """(bias, bn, scale64, shift64) of a layer: norm in none / bias / bn / bias+bn."""
    bias = ints(SEED, name + ".bias", (cout,), 1.0, 8).float() if "bias" in norm else None
    bn = pow2_bn(name + ".bn", cout, scales) if "bn" in norm else None
    scale, shift = fold64(cout, bias, bn)
    return bias, bn, scale, shift


def out_hw(H, W, k, stride, pad, transposed):
    if transposed:
        return 2 * H, 2 * W
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_chain(name, N, Cin, H, W, Cout, k=1, stride=1, pad=0, transposed=False, norm="bn", act="relu", res=False, pool=False, tail=0):
    """One conv / transposed conv with bias, BN, residual and activation; pool: the stem's 3x3 / s2 / p1 max-pool behind it; tail: a
    1x1 conv to `tail` channels with integer weights and bias behind the activation."""
    wshape = (Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)
    w = int_weights(name + ".w", wshape, 0.5, out_dim=1 if transposed else 0)
    x = int_input(name + ".x", (N, Cin, H, W))
    bias, bn, scale, shift = _epilogue(name, Cout, norm)
    Ho, Wo = out_hw(H, W, k, stride, pad, transposed)
    inputs = {"x": x}
    if res:
        inputs["r"] = ints(SEED, name + ".r", (N, Cout, Ho, Wo), 0.75, 16)
    post = (lambda v: F.max_pool2d(v, 3, 2, 1)) if pool else None
    layers = [Layer("t" if tail else "y", [Branch("x", w, stride, pad, transposed, scale)], shift, act, res="r" if res else None, post=post)]
    meta = {"w": w, "bias": bias, "bn": bn}
    if tail:
        wt = int_weights(name + ".wt", (tail, Cout, 1, 1), 16.0 / Cout)
        bt = ints(SEED, name + ".bt", (tail,), 1.0, 8)
        layers.append(Layer("y", [Branch("t", wt)], bt, None))
        meta.update(wt=wt, bt=bt)
    return Chain(name, inputs, layers, ["y"], stored=["t"] if tail else [], meta=meta)


def shortcut_chain(name, N, planes, cin, H, W, s):
    """relu(bn3(conv3(t2)) + bn_d(conv_d(x))): the K-concatenated shortcut conv (FusedShortcutConv)."""
    cout = 4 * planes
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    w3 = int_weights(name + ".w3", (cout, planes, 1, 1), 0.5)
    wd = int_weights(name + ".wd", (cout, cin, 1, 1), 0.5)
    bn3, bnd = pow2_bn(name + ".bn3", cout), pow2_bn(name + ".bnd", cout)
    (s3, sh3), (sd, shd) = fold64(cout, None, bn3), fold64(cout, None, bnd)
    inputs = {"t2": int_input(name + ".t2", (N, planes, Ho, Wo)), "x": int_input(name + ".x", (N, cin, H, W))}
    L = Layer("y", [Branch("t2", w3, scale=s3), Branch("x", wd, stride=s, scale=sd)], sh3 + shd, "relu")
    return Chain(name, inputs, [L], ["y"], meta={"w3": w3, "wd": wd, "bn3": bn3, "bnd": bnd})


BLOCK_SCALES = (1.0, -1.0, 1.0, -1.0)          # inside a block every t stays an integer
EXIT_SCALES = (1.0, -1.0, 0.5, -0.5)


def bottleneck_chain(name, N, H, W, P, C=None, kind="identity", stride2=1):
    """The fused blocks: kind identity (x + conv3), head (conv1 + conv2 only; stride2 = the stride of conv2), entry (projection
    shortcut K-concatenated with conv3) and exit (identity block, then the next stage's opening 1x1 conv + bn + relu on its output).
    Densities: about 64 / 72 / 16 non-zero weights per row of conv1 / conv2 / conv3 keep t1, t2, y well inside 2048."""
    C = C if C is not None else 4 * P
    w1 = int_weights(name + ".w1", (P, C, 1, 1), 64.0 / C)
    w2 = int_weights(name + ".w2", (P, P, 3, 3), 8.0 / P)
    bn1, bn2 = pow2_bn(name + ".bn1", P, BLOCK_SCALES, 3), pow2_bn(name + ".bn2", P, BLOCK_SCALES, 3)
    (s1, b1), (s2, b2) = fold64(P, None, bn1), fold64(P, None, bn2)
    inputs = {"x": int_input(name + ".x", (N, C, H, W))}
    layers = [Layer("t1", [Branch("x", w1, scale=s1)], b1, "relu"), Layer("t2", [Branch("t1", w2, stride2, 1, scale=s2)], b2, "relu")]
    meta = {"w1": w1, "w2": w2, "bn1": bn1, "bn2": bn2}
    if kind == "head":
        return Chain(name, inputs, layers, ["t2"], stored=["t1"], meta=meta)
    CO = 4 * P
    w3 = int_weights(name + ".w3", (CO, P, 1, 1), 16.0 / P)
    # (the exit form feeds y into one more conv: y stays an integer there, so that the tail's sums are exact up to 2048)
    bn3 = pow2_bn(name + ".bn3", CO, BLOCK_SCALES if kind == "exit" else EXIT_SCALES, 3)
    s3, b3 = fold64(CO, None, bn3)
    meta.update(w3=w3, bn3=bn3)
    if kind == "entry":
        wd = int_weights(name + ".wd", (CO, C, 1, 1), 16.0 / C)
        bnd = pow2_bn(name + ".bnd", CO, EXIT_SCALES, 3)
        sd, bd = fold64(CO, None, bnd)
        meta.update(wd=wd, bnd=bnd)
        layers.append(Layer("y", [Branch("t2", w3, scale=s3), Branch("x", wd, scale=sd)], b3 + bd, "relu"))
        return Chain(name, inputs, layers, ["y"], stored=["t1", "t2"], meta=meta)
    layers.append(Layer("y", [Branch("t2", w3, scale=s3)], b3, "relu", res="x"))
    if kind == "identity":
        return Chain(name, inputs, layers, ["y"], stored=["t1", "t2"], meta=meta)
    assert kind == "exit"
    T = 2 * P
    wt = int_weights(name + ".wt", (T, CO, 1, 1), 6.0 / CO)
    bnt = pow2_bn(name + ".bnt", T, BLOCK_SCALES, 3)
    st, bt = fold64(T, None, bnt)
    meta.update(wt=wt, bnt=bnt)
    layers.append(Layer("n1", [Branch("y", wt, scale=st)], bt, "relu"))
    return Chain(name, inputs, layers, ["y", "n1"], stored=["t1", "t2"], meta=meta)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _c(name, N, Cin, H, W, Cout, k=1, s=1, p=0, tr=False, norm="bn", act="relu", res=False, xoff=0, form=None, **kw):
    return dict(name=name, N=N, Cin=Cin, H=H, W=W, Cout=Cout, k=k, s=s, p=p, tr=tr, norm=norm, act=act, res=res, xoff=xoff, form=form, **kw)


# ft_conv_direct_fwd (fp16).  form: what ft_conv_direct_stream_id must say (test_exact_cases_cpu.py checks it against the library on the
# host): k1 / k4 / stationary = the 1x1 / gather kernel with K split 1 / 4 or weight-stationary, c3 = 3x3 whole maps or strips,
# c3s2 / c3s2_pair = 3x3 stride 2 with one / two images per workgroup (whole maps or strips), ws5 = 5x5 stride 2, deconv = transposed.
DIRECT_1X1 = [
    _c("ragged_pixels", 3, 256, 7, 5, 256, res=True, xoff=32, form="k4"),
    _c("ragged_pixels_wide", 5, 320, 9, 7, 512, xoff=32, form="k1"),
    _c("k2048_to_512_n3_8x6", 3, 2048, 8, 6, 512, xoff=32, form="k4"),
    _c("k512_to_2048_res_n3_8x6", 3, 512, 8, 6, 2048, res=True, xoff=32, form="k1"),
    _c("stationary_ragged", 7, 256, 97, 101, 256, xoff=32, form="stationary"),
]
# name, N, Hx, Wx, planes, cin_x, stride
DIRECT_SHORTCUT = [("stride1", 4, 9, 7, 256, 256, 1), ("l3_entry_small", 6, 32, 24, 256, 512, 2)]
DIRECT_3X3_WHOLE = [
    _c("tiny_3x5", 3, 512, 3, 5, 512, 3, 1, 1, form="c3"),
    _c("r101_12x9", 7, 512, 12, 9, 512, 3, 1, 1, form="c3"),
    _c("strips_ragged_last", 9, 512, 13, 16, 512, 3, 1, 1, form="c3"),
    _c("strips_w10", 9, 512, 20, 10, 512, 3, 1, 1, form="c3"),
    _c("c1024_tiny", 3, 1024, 2, 3, 1024, 3, 1, 1, form="c3"),
]
DIRECT_GATHER = [
    _c("odd_map_s2", 3, 256, 13, 9, 256, 3, 2, 1, form="k4"),
    _c("stride1_big_map", 2, 256, 20, 14, 256, 3, 1, 1, form="k4"),
    _c("long_walk", 2, 1024, 8, 6, 256, 3, 2, 1, form="k4"),
    _c("leaky_256_512_s2_slice", 2, 256, 12, 16, 512, 3, 2, 1, act="leaky", xoff=32, form="k4"),
    _c("ntile256_cin320_s2", 2, 320, 9, 7, 256, 3, 2, 1, act="leaky", xoff=32, form="k1"),     # Cin no multiple of 256: the N-tile 256 gather
    _c("s2_whole_odd_map", 3, 512, 13, 9, 512, 3, 2, 1, form="c3s2"),
    _c("s2_whole_one_tile", 5, 512, 8, 6, 128, 3, 2, 1, form="c3s2"),
    _c("s2_whole_16x16", 2, 512, 16, 16, 64, 3, 2, 1, form="c3s2"),
    _c("s2_pair_odd_batch", 51, 512, 12, 16, 512, 3, 2, 1, act="leaky", xoff=32, form="c3s2_pair"),
    _c("s2_pair_odd_map", 56, 512, 13, 9, 512, 3, 2, 1, form="c3s2_pair"),
    _c("s2_strips_ragged", 9, 512, 26, 20, 512, 3, 2, 1, xoff=32, form="c3s2"),
]
DIRECT_5X5 = [
    _c("ragged_patches", 3, 64, 41, 55, 128, 5, 2, 2, norm="bn", act="leaky", xoff=8, form="ws5"),
    _c("one_group", 2, 64, 30, 34, 64, 5, 2, 2, norm="bias", act="leaky", xoff=8, form="ws5"),
    _c("tiny_map", 5, 64, 5, 3, 256, 5, 2, 2, norm="bn", act="leaky", xoff=8, form="ws5"),
    _c("three_groups", 1, 64, 64, 48, 192, 5, 2, 2, norm="none", act="leaky", xoff=8, form="ws5"),
]
DIRECT_DECONV = [
    _c("n3_8x6_ragged_last_tile", 3, 256, 8, 6, 16, 4, 2, 1, tr=True, form="deconv"),
    _c("n5_6x8", 5, 320, 6, 8, 48, 4, 2, 1, tr=True, form="deconv"),
    _c("n9_4x3_ipw8", 9, 256, 4, 3, 256, 4, 2, 1, tr=True, form="deconv"),
    _c("n3_8x6_views", 3, 256, 8, 6, 48, 4, 2, 1, tr=True, xoff=32, yoff=64, form="deconv"),
]
DIRECT_CONVS = DIRECT_1X1 + DIRECT_3X3_WHOLE + DIRECT_GATHER + DIRECT_5X5 + DIRECT_DECONV


def direct_offsets(c):
    """((x channel stride, x channel offset), (y channel stride, y channel offset)) of a direct-conv case: the views of the existing
    tests of each family (test_conv_direct_gpu.py, test_deconv_direct_gpu.py), the output always a slice with guard channels on both sides."""
    if c["tr"]:
        yoff = c.get("yoff", 16)
        return (c["Cin"] + 2 * c["xoff"], c["xoff"]), (c["Cout"] + 2 * yoff, yoff)
    if c["k"] == 5:
        return (c["Cin"] + 16, 8), (c["Cout"] + 24, 16)
    if c["k"] == 1:
        return (c["Cin"] + 32, 32), (c["Cout"] + 96, 64)
    return (c["Cin"] + c["xoff"], c["xoff"]), (c["Cout"] + 64, 32)


def direct_weight_bytes(c):
    """Every form streams each fp16 weight once: 1x1 / gather K-split blocks of 32 KiB, the 3x3 whole-map fragments, the 5x5
    form's 200 KiB per 64 output channels and the transposed form's sixteen taps all come to this."""
    return 2 * c["k"] * c["k"] * c["Cin"] * c["Cout"]


def direct_form(stream_id, k, transposed):
    """Decode ft_conv_direct_stream_id (csrc/conv_direct.hip) into the names used above."""
    if stream_id < 0:
        return None
    top = stream_id >> 28
    if transposed:
        return "deconv" if top == 6 else "?"
    if k == 5:
        return "ws5" if top == 5 else "?"
    if top >= 4:
        return {4: "c3", 5: "c3s2", 7: "c3s2_pair"}.get(top, "?")
    return {1: "stationary", 2: "k1", 5: "k4"}.get(stream_id >> 24, "?")


# ft_conv2d_fwd: every tile variant, fp16 and fp32 (test_conv_gpu.VARIANT_CASES: bn + relu)
VARIANT_CONVS = [
    _c("var_1x1_res", 2, 128, 17, 13, 512, res=True),
    _c("var_3x3_s2_ragged", 2, 128, 15, 11, 128, 3, 2, 1),
    _c("var_3x3_ragged_cin96", 2, 96, 17, 13, 128, 3, 1, 1),
    _c("var_3x3_cin32_cout64", 1, 32, 20, 37, 64, 3, 1, 1),
    _c("var_deconv_cout64_wide_img", 1, 128, 6, 33, 64, 4, 2, 1, tr=True),
    _c("var_deconv_cin1026", 1, 1026, 5, 7, 256, 4, 2, 1, tr=True),
    _c("var_splitk_3x3_512", 2, 512, 8, 6, 512, 3, 1, 1),
    _c("var_splitk_1x1_res_k2048", 2, 2048, 8, 6, 512, res=True),
    _c("var_splitk_deconv_1024", 1, 1024, 6, 8, 512, 4, 2, 1, tr=True),
    _c("var_stem_pose_ragged", 3, 3, 36, 28, 64, 7, 2, 3),
    _c("var_stem_cs12_ragged", 2, 12, 50, 70, 64, 7, 2, 3),
    _c("var_stem_fusion_3x3", 2, 11, 19, 33, 64, 3, 1, 1),
    # the two smallest of test_conv8_gpu.CASES8 (the 8-phase tile is one of the hints; the odd K splits are added there)
    _c("1x1_128_two_ktiles", 2, 128, 17, 13, 256, norm="bias", act="leaky"),
    _c("3x3_cout1024_k4608", 1, 512, 6, 8, 1024, 3, 2, 1, norm="bias", act="leaky", odd_splits=True),
]
# forms with kernels of their own (test_conv_gpu.CASES / ROWPACK); layout as test_conv_matches_oracle names it
OWN_KERNEL_CONVS = [
    _c("fewout_cout3_5x5_s2", 1, 40, 11, 9, 3, 5, 2, 2, norm="bias", act="leaky", nchw_too=True),
    _c("fewout_cout4_1x1_res", 2, 64, 7, 5, 4, res=True),
    _c("predict_flow_patch_ragged_cout1", 3, 40, 70, 150, 1, 3, 1, 1, norm="bias", act="leaky"),
    _c("predict_flow_mfma_ragged_cout1", 5, 40, 70, 150, 1, 3, 1, 1, norm="bias", act="leaky"),
    _c("predict_flow_mfma_cin194", 6, 194, 64, 128, 2, 3, 1, 1, norm="bias", act=None, nchw_too=True),
    _c("persist_flow_conv1_6_ragged", 3, 6, 250, 500, 64, 7, 2, 3, norm="bias", act="leaky", packer=True),
    _c("conv_cin473", 1, 473, 8, 12, 256, 3, 1, 1, norm="bias", act="leaky", layout="tight"),
]
STEM_POOL = [("small_ragged_x", 2, 64, 48), ("ragged_xy", 3, 40, 56)]
# name, N, Cin, H, W, Cout, k, stride, pad, transposed, tail_cout: the two smallest of test_conv_gpu.TAIL_CASES and of test_conv8_gpu.TAIL8
TAILS = [("deconv128_tail32_ragged", 1, 64, 5, 7, 128, 4, 2, 1, True, 32), ("conv3x3_64_tail5", 2, 64, 9, 11, 64, 3, 1, 1, False, 5),
         ("conv1x1_256_tail1", 1, 512, 12, 10, 256, 1, 1, 0, False, 1), ("conv3x3_256_tail24", 2, 128, 20, 9, 256, 3, 1, 1, False, 24)]
# name, N, planes, Cin of the block input, H, W, stride: one of test_conv_gpu.SHORTCUT_CASES per stride
SHORTCUTS = [("layer1_like", 2, 64, 64, 16, 12, 1), ("odd_channels", 1, 96, 160, 10, 6, 2)]

# bottleneck entry points: name, N, H, W, x channel stride, x channel offset, planes
PATCH_BLOCKS = [("ragged_xy_13x20", 3, 13, 20, 256, 0, 64), ("tiny_5x3", 1, 5, 3, 256, 0, 64), ("view_offset", 1, 16, 16, 320, 32, 64)]
RSTAT_BLOCKS = [("rs_tiny_5x3", 1, 5, 3, 256, 0, 64, 5), ("rs_view_offset", 1, 16, 16, 320, 32, 64, 7)]            # + rows per strip
S128_BLOCKS = [("s128_ragged_13x20", 2, 13, 20, 512, 0, 128), ("s128_tiny_5x3", 1, 5, 3, 512, 0, 128), ("s128_view_offset", 1, 16, 16, 576, 32, 128),
               ("s128_wide_60", 1, 6, 60, 512, 0, 128)]
S256_BLOCKS = [("s256_tiny_5x3", 1, 5, 3, 1024, 0, 256), ("s256_view_offset", 1, 9, 7, 1056, 32, 256), ("s256_odd_width_11x9", 3, 11, 9, 1024, 0, 256),
               ("s256_wide_6x40", 2, 6, 40, 1024, 0, 256)]
T16_BLOCKS = [("t16_tiny_5x3", 1, 5, 3, 1024, 0, 256), ("t16_view_offset_9x7", 1, 9, 7, 1056, 32, 256)]
D128_BLOCKS = [("d128_tiny_5x3", 1, 5, 3, 512, 0, 128), ("d128_view_offset_9x7", 1, 9, 7, 544, 32, 128)]
CLUSTER_BLOCKS = [("c256_view_offset_10x7", 3, 10, 7, 1056, 32, 256), ("c256_tiny_6x3", 1, 6, 3, 1024, 0, 256)]
HEAD_BLOCK = ("ragged_13x20", 3, 13, 20)                                   # 64 -> 64 -> 64
HEAD2_BLOCK = ("h2_tiny_4x2", 1, 4, 2, 512, 0)                             # 512 -> 256 -> 256, stride 2 on conv2
ENTRY_BLOCK = ("view_out", 2, 16, 16)                                      # 64 -> 64 -> 64 -> 256 with the projection shortcut
EXIT_BLOCKS = [("single_patch_8x16", 1, 8, 16, 256, 0, 128, 0, "even"), ("views_16x16", 2, 16, 16, 320, 32, 192, 32, "even")]
IDENTITY_BLOCKS = PATCH_BLOCKS + [b[:7] for b in RSTAT_BLOCKS] + S128_BLOCKS + S256_BLOCKS + T16_BLOCKS + D128_BLOCKS + CLUSTER_BLOCKS


@functools.lru_cache(maxsize=None)
def conv_case(name):
    c = next(c for c in DIRECT_CONVS + VARIANT_CONVS + OWN_KERNEL_CONVS if c["name"] == name)
    return conv_chain(name, c["N"], c["Cin"], c["H"], c["W"], c["Cout"], c["k"], c["s"], c["p"], c["tr"], c["norm"], c["act"], c["res"])


@functools.lru_cache(maxsize=None)
def direct_shortcut_case(name):
    _, N, Hx, Wx, planes, cin_x, s = next(c for c in DIRECT_SHORTCUT if c[0] == name)
    return shortcut_chain("direct." + name, N, planes, cin_x, Hx, Wx, s)


@functools.lru_cache(maxsize=None)
def shortcut_case(name):
    _, N, planes, cin, H, W, s = next(c for c in SHORTCUTS if c[0] == name)
    return shortcut_chain(name, N, planes, cin, H, W, s)


@functools.lru_cache(maxsize=None)
def stem_pool_case(name):
    _, N, H, W = next(c for c in STEM_POOL if c[0] == name)
    return conv_chain("stempool." + name, N, 3, H, W, 64, 7, 2, 3, norm="bn", act="relu", pool=True)


@functools.lru_cache(maxsize=None)
def tail_case(name):
    _, N, Cin, H, W, Cout, k, s, p, tr, nt = next(c for c in TAILS if c[0] == name)
    return conv_chain("tail." + name, N, Cin, H, W, Cout, k, s, p, tr, norm="bn", act="relu", tail=nt)


@functools.lru_cache(maxsize=None)
def block_case(name):
    if name == "head." + HEAD_BLOCK[0]:
        return bottleneck_chain(name, *HEAD_BLOCK[1:], 64, C=64, kind="head")
    if name == "head2." + HEAD2_BLOCK[0]:
        return bottleneck_chain(name, *HEAD2_BLOCK[1:4], 256, C=512, kind="head", stride2=2)
    if name == "entry." + ENTRY_BLOCK[0]:
        return bottleneck_chain(name, *ENTRY_BLOCK[1:], 64, C=64, kind="entry")
    for e in EXIT_BLOCKS:
        if name == "exit." + e[0]:
            return bottleneck_chain(name, e[1], e[2], e[3], 64, kind="exit")
    _, N, H, W, _, _, P = next(b for b in IDENTITY_BLOCKS if b[0] == name)
    return bottleneck_chain(name, N, H, W, P)


def all_cases():
    """(id, zero-argument constructor) of every chain the GPU tests use."""
    out = [(c["name"], functools.partial(conv_case, c["name"])) for c in DIRECT_CONVS + VARIANT_CONVS + OWN_KERNEL_CONVS]
    out += [("direct_shortcut." + c[0], functools.partial(direct_shortcut_case, c[0])) for c in DIRECT_SHORTCUT]
    out += [("shortcut." + c[0], functools.partial(shortcut_case, c[0])) for c in SHORTCUTS]
    out += [("stempool." + c[0], functools.partial(stem_pool_case, c[0])) for c in STEM_POOL]
    out += [("tail." + c[0], functools.partial(tail_case, c[0])) for c in TAILS]
    names = [b[0] for b in IDENTITY_BLOCKS] + ["head." + HEAD_BLOCK[0], "head2." + HEAD2_BLOCK[0], "entry." + ENTRY_BLOCK[0]] + ["exit." + e[0] for e in EXIT_BLOCKS]
    out += [(n, functools.partial(block_case, n)) for n in names]
    return out


# ---- what the CPU test asks of every case ----------------------------------------------------------------------------------------------
def tensor_report(chain):
    """(max magnitude, zero share of the outputs) after asserting that everything a kernel stores in fp16 is representable."""
    T = chain.T
    mx = 0.0
    for k in list(chain.inputs) + list(chain.stored) + list(chain.outputs):
        t = T[k]
        assert torch.equal(t.half().double(), t), f"{chain.name}: {k} is not exact in fp16"
        mx = max(mx, t.abs().max().item())
    for L in chain.layers:
        mx = max(mx, T["pre:" + L.out].abs().max().item())
    zeros = max((T[o] == 0).double().mean().item() for o in chain.outputs)
    return mx, zeros


def _input_pos(b, oy, ox, ky, kx, Hi, Wi):
    if b.transposed:
        ty, tx = oy + b.pad - ky, ox + b.pad - kx
        if ty % b.stride or tx % b.stride:
            return None
        iy, ix = ty // b.stride, tx // b.stride
    else:
        iy, ix = oy * b.stride - b.pad + ky, ox * b.stride - b.pad + kx
    return (iy, ix) if 0 <= iy < Hi and 0 <= ix < Wi else None


def teeth(chain, count=16):
    """Drop one product / count it twice at `count` pseudo-random (layer, pixel, tap, channel) positions — among them the last channel,
    the last tap and a border pixel — and require the reference to change each time.  The product is taken at a non-zero input value;
    the output channel is the first (from a pseudo-random start) whose weight is non-zero and whose change the activation does not
    hide.  Returns the number of positions tried."""
    T = chain.T
    slots = [(li, bi) for li, L in enumerate(chain.layers) for bi in range(len(L.branches))]
    tried = 0
    for t in range(count):
        li, bi = slots[t % len(slots)]
        L, b = chain.layers[li], chain.layers[li].branches[bi]
        x, pre = T[b.src], T["pre:" + L.out]
        N, Ci, Hi, Wi = x.shape
        _, Co, Ho, Wo = pre.shape
        k = b.w.shape[2]
        kind = {0: "last_channel", 1: "last_tap", 2: "border"}.get(t // len(slots), "any") if t < 3 * len(slots) else "any"
        u = synth.uniform(SEED, f"{chain.name}.teeth{t}", (256, 7)).double()
        found = False
        for r in u:
            n, oy, ox, ky, kx, ci, co0 = (int(v * m) for v, m in zip(r.tolist(), (N, Ho, Wo, k, k, Ci, Co)))
            if kind == "last_channel":
                ci = Ci - 1
            elif kind == "last_tap":
                ky = kx = k - 1
            elif kind == "border":
                oy, ox = (0, ox) if ky % 2 else (oy, 0)
            pos = _input_pos(b, oy, ox, ky, kx, Hi, Wi)
            if pos is None or x[n, ci, pos[0], pos[1]] == 0:
                continue
            wcol = b.w[ci, :, ky, kx] if b.transposed else b.w[:, ci, ky, kx]
            for co in [(co0 + j) % Co for j in range(Co)]:
                if wcol[co] == 0:
                    continue
                delta = x[n, ci, pos[0], pos[1]] * wcol[co] * (b.scale[co] if b.scale is not None else 1.0)
                ok = all(any(not torch.equal(a, c) for a, c in chain.tampered(li, (n, co, oy, ox), sgn * delta)) for sgn in (-1.0, 1.0))
                if ok:
                    found = True
                    break
                if li < len(chain.layers) - 1:
                    break           # (a hidden change inside a chain: take another position rather than recompute per channel)
            if found:
                break
        assert found, f"{chain.name}: no visible product found for position {t} ({kind}, layer {li}, branch {bi})"
        tried += 1
    return tried


def coverage(chain):
    """Every (tap, input channel) column and every output channel of every weight tensor is non-zero; every image has non-zero input
    in every channel."""
    for L in chain.layers:
        for b in L.branches:
            w = b.w.movedim(1, 0) if b.transposed else b.w
            assert bool((w.abs().sum(0) > 0).all()), f"{chain.name}: an all-zero weight column feeding {L.out}"
            assert bool((w.abs().sum((1, 2, 3)) > 0).all()), f"{chain.name}: an output channel of {L.out} without a weight"
    for k, x in chain.inputs.items():
        if k != "r":
            assert bool((x.abs().sum((2, 3)) > 0).all()), f"{chain.name}: input {k} has an all-zero channel in some image"


# ---- helpers of the GPU tests ----------------------------------------------------------------------------------------------------------
X_POISON, Y_POISON = 7.0, 3.0


def input_view(x64, dtype, dev, cstride=None, coff=0):
    """The input as a channel slice [coff, coff + C) of an NHWC buffer; the channels in front of the slice hold X_POISON."""
    from util import nchw_to_view
    v = nchw_to_view(x64.float(), dtype, dev, cstride=cstride, coff=coff)
    if coff:
        v.t[..., :coff] = X_POISON
    return v


def output_view(N, H, W, C, dtype, dev, cstride, coff):
    """A poisoned NHWC buffer whose channels [coff, coff + C) the launch may write."""
    from flowtrack.pytorch_amd.hip_ops import ActView
    assert coff > 0 and cstride > coff + C, "guard channels on both sides"
    return ActView(torch.full((N, H, W, cstride), Y_POISON, dtype=dtype, device=dev), C, coff)


def assert_guards(y, what):
    assert torch.all(y.t[..., :y.coff] == Y_POISON) and torch.all(y.t[..., y.coff + y.C:] == Y_POISON), f"{what}: channels outside the output slice were written"


def assert_exact(got, want, what):
    """Element for element (+-0 are equal)."""
    got = got.double().cpu()
    if not torch.equal(got, want):
        bad = (got != want)
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 reference, max |diff| "
                             f"{(got - want).abs().max().item():g}; first at {i}: got {got[i].item():g}, want {want[i].item():g}")
