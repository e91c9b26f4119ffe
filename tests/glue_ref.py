"""High-precision CPU references for the small kernels between the convs ("glue"): the fused warp / concat stages of the stacked
FlowNets, the x4 upsamplers, the 3x3/s2 max-pool and the NCHW <-> NHWC packers.  TEST INFRASTRUCTURE ONLY.

The two concat stages restate Resample2d's rule (Resample2d_kernel.cu:42-59): the sample position x + dx and the two
fractions are formed in float32 exactly as the reference's kernel forms them (so the taps and weights are the reference's, not
those of an exact-arithmetic warp), weights come from the UNclamped floor, neighbour indices are clamped to the frame, nothing is
renormalised.  Everything behind the fractions — weights, products, differences, norms, flow / div_flow — is float64.
tests/test_glue_cpu.py pins both against the C restatement of the reference operators (oracle/ops_ref.py)."""
import numpy as np
import torch
import torch.nn.functional as F


def warp_ref(img, flow):
    """Resample2d of img [B,C,H,W] (any float, read as float64) by flow [B,2,H,W] (float32) -> float64 [B,C,H,W]."""
    img = np.asarray(img, dtype=np.float64)
    flow = np.asarray(flow, dtype=np.float32)
    B, C, H, W = img.shape
    assert flow.shape == (B, 2, H, W)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    xf = xx[None] + flow[:, 0]                      # float32 sums, as the kernels form them
    yf = yy[None] + flow[:, 1]
    assert xf.dtype == np.float32 and yf.dtype == np.float32
    fx, fy = np.floor(xf), np.floor(yf)
    a = (xf - fx).astype(np.float64)[:, None]       # float32 differences, rounded as the kernels round them, then widened
    b = (yf - fy).astype(np.float64)[:, None]
    xL = np.clip(fx, 0, W - 1).astype(np.int64)[:, None]          # clamped in float first: 1e9 never meets an integer conversion
    xR = np.clip(fx + 1, 0, W - 1).astype(np.int64)[:, None]
    yT = np.clip(fy, 0, H - 1).astype(np.int64)[:, None]
    yB = np.clip(fy + 1, 0, H - 1).astype(np.int64)[:, None]
    bi = np.arange(B)[:, None, None, None]
    ci = np.arange(C)[None, :, None, None]
    return ((1 - a) * (1 - b) * img[bi, ci, yT, xL] + a * (1 - b) * img[bi, ci, yT, xR]
            + (1 - a) * b * img[bi, ci, yB, xL] + a * b * img[bi, ci, yB, xR])


def _norm(x):
    return np.sqrt((x * x).sum(1, keepdims=True))


def warp_concat_ref(x6, flow, div_flow):
    """(img0, img1, warp(img1, flow), flow / div_flow, ||img0 - warp||_2): float64 [B,12,H,W] (models.py:396-403)."""
    x6 = np.asarray(x6, dtype=np.float64)
    flow32 = np.asarray(flow, dtype=np.float32)
    w = warp_ref(x6[:, 3:6], flow32)
    return np.concatenate((x6, w, flow32.astype(np.float64) / float(div_flow), _norm(x6[:, :3] - w)), axis=1)


def fusion_concat_ref(x6, flow_sd, flow_s2):
    """(img0, flow_sd, flow_s2, |flow_sd|, |flow_s2|, ||img0 - warp(img1, flow_sd)||, ||img0 - warp(img1, flow_s2)||):
    float64 [B,11,H,W] (models.py:140-168, concat3)."""
    x6 = np.asarray(x6, dtype=np.float64)
    sd32, s232 = np.asarray(flow_sd, dtype=np.float32), np.asarray(flow_s2, dtype=np.float32)
    sd, s2 = sd32.astype(np.float64), s232.astype(np.float64)
    img0, img1 = x6[:, :3], x6[:, 3:6]
    return np.concatenate((img0, sd, s2, _norm(sd), _norm(s2), _norm(img0 - warp_ref(img1, sd32)), _norm(img0 - warp_ref(img1, s232))),
                          axis=1)


# ---- the remaining references are torch itself ------------------------------------------------------------------------------
def upsample_bilinear4x_ref(x, mul):
    """nn.Upsample(scale_factor=4, mode='bilinear') of x * mul, in float64."""
    return F.interpolate(x.double() * float(mul), scale_factor=4, mode="bilinear", align_corners=False)


def upsample_nearest4x_ref(x, mul):
    """nn.Upsample(scale_factor=4, mode='nearest') of x * float32(mul): one fp32 product per element, then copies."""
    return F.interpolate(x.float() * np.float32(mul), scale_factor=4, mode="nearest")


def maxpool3x3s2_ref(x_nhwc):
    """nn.MaxPool2d(3, 2, 1) on NHWC values (fp32 holds every fp16 value and a maximum selects: exact in either dtype;
    a NaN in the window gives NaN, the padding is -inf)."""
    return F.max_pool2d(x_nhwc.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def pack_ref(x_nchw, cpad, lpad, wpitch, dtype):
    """NCHW fp32 -> NHWC `dtype` [N,H,wpitch,cpad]: pixel x in column lpad + x, everything else zero."""
    N, C, H, W = x_nchw.shape
    y = torch.zeros((N, H, wpitch, cpad), dtype=dtype)
    y[:, :, lpad:lpad + W, :C] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    return y


def unpack_ref(x_nhwc, C, coff):
    """Channel slice [coff, coff + C) of an NHWC buffer -> NCHW fp32."""
    return x_nhwc[..., coff:coff + C].permute(0, 3, 1, 2).float().contiguous()


# ---- shared inputs of the concat tests ---------------------------------------------------------------------------------------
DIV_FLOW = 20.0
# (B, H, W, x_lpad, x_wpitch, y_lpad, y_wpitch)
CONCAT_SHAPES = [
    (2, 9, 13, 0, 13, 0, 13),        # plain NHWC; 234 physical pixels: less than a workgroup, no multiple of 64
    (3, 17, 61, 3, 68, 3, 68),       # the layout the models use (pad 3); total % 64 != 0: the fp16 store's fallback for the last wave
    (2, 24, 40, 3, 46, 1, 42),       # different pads in and out
    (1, 50, 130, 2, 140, 5, 144),    # several workgroups, spare columns on the right
    (2, 1, 7, 0, 7, 0, 8),           # one row: every vertical tap clamps
    (2, 6, 1, 1, 4, 0, 2),           # one column: every horizontal tap clamps
    (4, 16, 64, 0, 64, 0, 64),       # total a multiple of 256: every wave whole
]
BIG_SHAPE = (5, 832, 1024, 3, 1030, 3, 1030)   # past the 16384-block grid cap, see test_glue_gpu.py


def planted_vectors(fp16):
    """The flow vectors every map carries at fixed valid positions: far out of frame both ways, zero, an integer shift; the fp32
    cases add one beyond any integer conversion (fp16 keeps |flow| <= 3000 so that flow / div_flow and |flow| stay finite in fp16)."""
    v = [(-1000.0, 2500.0), (3000.0, -3000.0), (0.0, 0.0), (1.0, -2.0)]
    return v if fp16 else v + [(1e9, -1e9)]


def make_flow(seed, name, B, H, W, fp16):
    """[B,2,H,W] float32: N(0, 4 px) vectors, about 5 % of them 40 times longer, plus planted_vectors in every map."""
    from flowtrack.pytorch_amd import synth
    flow = (synth.normal(seed, name, (B, 2, H, W)) * 4.0).numpy()
    far = synth.uniform(seed, name + ".far", (B, 1, H, W), 0.0, 1.0).numpy() < 0.05
    flow = np.where(far, flow * 40.0, flow).astype(np.float32)
    vecs = planted_vectors(fp16)
    n = H * W
    for b in range(B):
        for k, v in enumerate(vecs):
            pos = (((2 * k + 1) * n) // (2 * len(vecs)) + b) % n       # spread over the map, another pixel in every batch entry
            flow[b, :, pos // W, pos % W] = v
    return flow


def make_images(seed, name, B, H, W, fp16):
    """[B,6,H,W] float32 ~ N(0, 0.5); for fp16 rounded to fp16 first (the reference reads what the kernel reads)."""
    from flowtrack.pytorch_amd import synth
    x = synth.normal(seed, name, (B, 6, H, W)) * 0.5
    return (x.half().float() if fp16 else x).numpy()
