"""Deterministic synthetic inputs and weights (no dependence on torch / numpy RNG streams).

Every tensor is a pure function of (seed, name, shape): a counter-based integer hash (splitmix64
finaliser) mapped to floats, so the oracle side, the HIP side and the golden-vector generator
regenerate bit-identical tensors and only OUTPUTS need to be committed as fixtures.

`fill_pose_state_dict` / `fill_flow_state_dict` write a NON-degenerate weight set: the reference's
default init gives |heatmap| ~ 1e-4 (deconv / heatmap std 0.001, pose_deconv.py:53,62), which would
make a 1e-3 tolerance vacuous and the arg-max a coin flip.
"""
from __future__ import annotations

import zlib
from typing import Dict, Tuple

import numpy as np
import torch

_M = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _key(seed: int, name: str, stream: int) -> np.uint64:
    h = zlib.crc32(name.encode()) & 0xFFFFFFFF
    return np.uint64(((seed & 0xFFFF) << 48) ^ (h << 16) ^ (stream & 0xFFFF))


def uniform01(seed: int, name: str, shape, stream: int = 0) -> np.ndarray:
    """float64 in [0, 1), shape `shape`."""
    n = int(np.prod(shape)) if len(shape) else 1
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + _mix(np.array([_key(seed, name, stream)], dtype=np.uint64))
    bits = _mix(ctr)
    return ((bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)).reshape(shape)


def uniform(seed: int, name: str, shape, lo: float = 0.0, hi: float = 1.0) -> torch.Tensor:
    return torch.from_numpy((lo + (hi - lo) * uniform01(seed, name, shape)).astype(np.float32))


def normal(seed: int, name: str, shape, std: float = 1.0, mean: float = 0.0) -> torch.Tensor:
    u1 = uniform01(seed, name, shape, stream=1)
    u2 = uniform01(seed, name, shape, stream=2)
    z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
    return torch.from_numpy((mean + std * z).astype(np.float32))


# ---- inputs ---------------------------------------------------------------------------------------
def pose_crops(seed: int, B: int, H: int = 256, W: int = 192) -> torch.Tensor:
    """[B,3,H,W] ~ N(0,1): the statistics of a mean/std-normalised crop (coco.py:152)."""
    return normal(seed, "pose_crops", (B, 3, H, W))


def frame_pairs(seed: int, B: int, H: int = 384, W: int = 512, max_shift: int = 8) -> torch.Tensor:
    """[B,3,2,H,W] in [0,255]: smooth-ish random texture; frame 1 = frame 0 translated by a known
    integer shift (|s| <= max_shift, per sample) plus N(0,2) noise, so the flow is meaningful."""
    pad = max_shift
    lo = uniform01(seed, "frame_lo", (B, 3, (H + 2 * pad) // 8 + 2, (W + 2 * pad) // 8 + 2))
    base = np.kron(lo, np.ones((1, 1, 8, 8)))[:, :, :H + 2 * pad, :W + 2 * pad]
    fine = uniform01(seed, "frame_fine", (B, 3, H + 2 * pad, W + 2 * pad))
    canvas = 255.0 * (0.7 * base + 0.3 * fine)
    shifts = np.floor(uniform01(seed, "frame_shift", (B, 2)) * (2 * max_shift + 1)).astype(np.int64) - max_shift
    noise = normal(seed, "frame_noise", (B, 3, H, W), std=2.0).numpy().astype(np.float64)
    out = np.empty((B, 3, 2, H, W), dtype=np.float32)
    for b in range(B):
        sy, sx = int(shifts[b, 0]), int(shifts[b, 1])
        out[b, :, 0] = canvas[b, :, pad:pad + H, pad:pad + W]
        out[b, :, 1] = np.clip(canvas[b, :, pad + sy:pad + sy + H, pad + sx:pad + sx + W] + noise[b], 0.0, 255.0)
    return torch.from_numpy(out)


def flow_field(seed: int, B: int, H: int, W: int, magnitude: float = 6.0) -> torch.Tensor:
    """[B,2,H,W] fp32 sub-pixel flow for warp tests, including out-of-frame targets."""
    return normal(seed, "flow_field", (B, 2, H, W), std=magnitude)


def peaked_heatmaps(seed: int, N: int, K: int = 17, h: int = 64, w: int = 48, sigma: float = 2.0, noise: float = 1e-3) -> torch.Tensor:
    """[N,K,h,w] heat maps shaped like a TRAINED pose net's output: one Gaussian bump per map with the training target's sigma
    (lib/pose/utils/heatmap.py:19-60: exp(-d^2 / (2 sigma^2)), sigma = 2 map pixels, tools/pose/config.py:85), amplitude
    0.7 .. 1.0, its centre at a uniformly random SUB-PIXEL position (a joint does not sit on the 4-pixel grid of the map), plus
    N(0, noise^2) of background.  The top-1 / top-2 margin of such a map is ~ amplitude * (1 - 2 |offset|) / (2 sigma)^2 per axis:
    near-ties between the two pixels that straddle the centre are a property of the maps, not of the arithmetic."""
    cy = 4.0 + uniform01(seed, "peak.cy", (N, K)) * (h - 8.0)
    cx = 4.0 + uniform01(seed, "peak.cx", (N, K)) * (w - 8.0)
    amp = 0.7 + 0.3 * uniform01(seed, "peak.amp", (N, K))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d2 = (yy[None, None] - cy[..., None, None]) ** 2 + (xx[None, None] - cx[..., None, None]) ** 2
    hm = amp[..., None, None] * np.exp(-d2 / (2.0 * sigma * sigma))
    return torch.from_numpy(hm.astype(np.float32)) + noise * normal(seed, "peak.noise", (N, K, h, w))


# ---- weights ---------------------------------------------------------------------------------------
def _fan_in(name: str, shape: Tuple[int, ...], transposed: bool) -> int:
    if transposed:  # [Cin, Cout, 4, 4]; every output pixel sees 2x2 of the 4x4 taps
        return shape[0] * 4
    return shape[1] * shape[2] * shape[3]


def fill_pose_state_dict(sd: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """He-scaled conv / deconv / heatmap weights and randomised BN statistics for a
    `deconv('resnetNN', K)` state_dict (keys as SURVEY Appendix B). bn3 / downsample gammas are kept
    small so 16-33 residual blocks do not blow the activations out of fp16 range."""
    out = {}
    for k, v in sd.items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            out[k] = normal(seed, k, shape, std=0.1)
        elif k.endswith("running_var"):
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif v.dim() == 4:
            transposed = k.startswith("deconv.")
            gain = 1.0 if k.startswith("heatmap") else 2.0
            std = float(np.sqrt(gain / _fan_in(k, shape, transposed)))
            out[k] = normal(seed, k, shape, std=std)
        elif k.endswith(".weight"):  # BN gamma
            last = ".bn3." in k or ".downsample.1." in k
            out[k] = uniform(seed, k, shape, 0.2, 0.4) if last else uniform(seed, k, shape, 0.5, 1.5)
        elif k.endswith(".bias"):
            out[k] = normal(seed, k, shape, std=0.1)
        else:
            raise KeyError(k)
    return out


#: conv gains of fill_densenet_state_dict (He's 2.0 in fill_pose_state_dict): every conv but the last, and the heat-map conv
DENSENET_GAIN, DENSENET_HEATMAP_GAIN = 1.0, 9.0


def fill_densenet_state_dict(sd: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Weights for an `fpn_densenet('densenetNNN', K)` state_dict: fill_pose_state_dict's recipe with every conv at gain
    DENSENET_GAIN and the heat-map conv at DENSENET_HEATMAP_GAIN.  A dense block has no BatchNorm behind a layer's last conv and concatenates instead of adding, so with He gains
    the FPN head's four lateral convs sum over up to 1024 un-normalised channels and the heat maps span about -53 .. 37: too wide
    for an absolute 1e-3 bound in fp32.  Gain 1 everywhere gives maps within +-3 whose top-1 / top-2 margins are too small for an
    exact arg-max test; the heat-map conv's gain stretches them to about +-10 (tests/golden/make_fpn_densenet_golden.py states the conditions this fill meets)."""
    out = {}
    for k, v in sd.items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            out[k] = normal(seed, k, shape, std=0.1)
        elif k.endswith("running_var"):
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif v.dim() == 4:
            gain = DENSENET_HEATMAP_GAIN if k.startswith("heatmap") else DENSENET_GAIN
            out[k] = normal(seed, k, shape, std=float(np.sqrt(gain / _fan_in(k, shape, False))))
        elif k.endswith(".weight"):  # BN gamma
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif k.endswith(".bias"):
            out[k] = normal(seed, k, shape, std=0.1)
        else:
            raise KeyError(k)
    return out


#: gain of the hourglass convs that write into the residual stream (fill_hg_state_dict)
HG_STREAM_GAIN = 0.03


def fill_hg_state_dict(sd: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Weights for an `hg(K, num_stacks)` state_dict.  The hourglass has no BatchNorm behind a block's last conv, so He gains
    everywhere let the residual stream grow with every one of its 112 blocks (the reference reaches 1e19 after 8 stacks).  The convs
    that write into that stream — every block's last conv (`*.branch.6`), `proj_` and `heatmap_` — therefore take the small gain
    HG_STREAM_GAIN, the heat-map convs 1.0 and every other conv the usual 2.0; BatchNorm statistics and biases as in
    fill_pose_state_dict."""
    out = {}
    for k, v in sd.items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            out[k] = normal(seed, k, shape, std=0.1)
        elif k.endswith("running_var"):
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif v.dim() == 4:
            if ".branch.6." in k or k.startswith("proj_.") or k.startswith("heatmap_."):
                gain = HG_STREAM_GAIN
            else:
                gain = 1.0 if k.startswith("heatmap.") else 2.0
            out[k] = normal(seed, k, shape, std=float(np.sqrt(gain / _fan_in(k, shape, False))))
        elif k.endswith(".weight"):  # BN gamma
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif k.endswith(".bias"):
            out[k] = normal(seed, k, shape, std=0.1)
        else:
            raise KeyError(k)
    return out


#: gains of fill_detector_state_dict: the block-closing BatchNorms of the trunk, and the He-style gains (std = sqrt(gain / fan_in)) of
#: the detector's head layers, chosen so that no softmax saturates and every box delta stays below 1 (tests/golden/make_detect_net_golden.py
#: checks the conditions on the reference's own run)
DET_BN_LAST = (0.1, 0.25)
DET_HEAD_GAINS = {"rpn_net": 2.0, "rpn_cls_score_net": 1.0, "rpn_bbox_pred_net": 0.008, "cls_score_net": 8.0, "bbox_pred_net": 4.0}


def fill_detector_state_dict(sd: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Weights for a detection.nets.resnetv1 state_dict: the trunk as fill_pose_state_dict fills it, with smaller gains on the
    BatchNorms that close a block (13 residual blocks feed net_conv with no normalisation behind them); the five head layers
    (`rpn_*`, `cls_score_net`, `bbox_pred_net`; two of them Linear, whose 2-D weights are NOT BatchNorm gains) N(0, gain / fan_in)
    with DET_HEAD_GAINS and small biases."""
    out = {}
    for k, v in sd.items():
        shape = tuple(v.shape)
        head = k.split(".")[0]
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            out[k] = normal(seed, k, shape, std=0.1)
        elif k.endswith("running_var"):
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif head in DET_HEAD_GAINS:
            if k.endswith(".weight"):
                out[k] = normal(seed, k, shape, std=float(np.sqrt(DET_HEAD_GAINS[head] / int(np.prod(shape[1:])))))
            else:
                out[k] = normal(seed, k, shape, std=0.05)
        elif v.dim() == 4:
            out[k] = normal(seed, k, shape, std=float(np.sqrt(2.0 / _fan_in(k, shape, False))))
        elif k.endswith(".weight"):  # BN gamma
            last = ".bn3." in k or ".downsample.1." in k
            out[k] = uniform(seed, k, shape, *DET_BN_LAST) if last else uniform(seed, k, shape, 0.5, 1.5)
        elif k.endswith(".bias"):
            out[k] = normal(seed, k, shape, std=0.1)
        else:
            raise KeyError(k)
    return out


#: gains (std = sqrt(gain / fan_in)) of fill_vgg_detector_state_dict's trunk: the first conv reads mean-subtracted pixels of
#: magnitude ~100 and scales them down by 20; the twelve convs behind it keep He's 2.0 (no BatchNorm: nothing else holds the
#: magnitude), which leaves |net_conv| near 20 and the RPN's deltas spread enough for its NMS to keep tens of boxes; the two
#: classifier layers shrink it again so that the class softmax does not saturate (tests/golden/make_detect_vgg_golden.py checks
#: the conditions on the reference's run)
VGG_FIRST_CONV_GAIN = 2.0 / 400.0
VGG_CONV_GAIN = 2.0
VGG_FC_GAIN = 0.4


def fill_vgg_detector_state_dict(sd: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Weights for a detection.nets.vgg16 state_dict.  `vgg.features.*` convs N(0, gain / fan_in) with the gains above and N(0, 0.05)
    biases (there is no BatchNorm in this trunk); the two `vgg.classifier.*` weights from ONE uniform stream each, U(-a, a) with
    a = sqrt(3 gain / fan_in), the variance of the wanted normal (synth.normal draws two streams and takes 12 s and three times
    the memory on the 4096 x 25088 matrix); the five head layers as fill_detector_state_dict fills them."""
    out = {}
    for k, v in sd.items():
        shape = tuple(v.shape)
        head = k.split(".")[0]
        if head in DET_HEAD_GAINS:
            if k.endswith(".weight"):
                out[k] = normal(seed, k, shape, std=float(np.sqrt(DET_HEAD_GAINS[head] / int(np.prod(shape[1:])))))
            else:
                out[k] = normal(seed, k, shape, std=0.05)
        elif k.startswith("vgg.features.") and v.dim() == 4:
            gain = VGG_FIRST_CONV_GAIN if k == "vgg.features.0.weight" else VGG_CONV_GAIN
            out[k] = normal(seed, k, shape, std=float(np.sqrt(gain / _fan_in(k, shape, False))))
        elif k.startswith("vgg.classifier.") and v.dim() == 2:
            a = float(np.sqrt(3.0 * VGG_FC_GAIN / shape[1]))
            out[k] = uniform(seed, k, shape, -a, a)
        elif k.endswith(".bias"):
            out[k] = normal(seed, k, shape, std=0.05)
        else:
            raise KeyError(k)
    return out


def detector_frame(seed: int, H: int, W: int) -> np.ndarray:
    """uint8 [H,W,3] BGR: a smooth random texture (8 x 8 blocks, 70 %) under fine noise (30 %), as frame_pairs builds its frames."""
    lo = uniform01(seed, "det_frame_lo", (H // 8 + 2, W // 8 + 2, 3))
    base = np.kron(lo, np.ones((8, 8, 1)))[:H, :W]
    fine = uniform01(seed, "det_frame_fine", (H, W, 3))
    return np.clip(np.floor(255.0 * (0.7 * base + 0.3 * fine)), 0, 255).astype(np.uint8)


def fill_flow_state_dict(sd: Dict[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """He-scaled (LeakyReLU 0.1) conv / deconv weights and small biases for a FlowNet2* state_dict."""
    out = {}
    for k, v in sd.items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            out[k] = normal(seed, k, shape, std=0.1)
        elif k.endswith("running_var"):
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        elif v.dim() == 4:
            leaf = k.split(".")[-2] if k.split(".")[-2] != "0" else k.split(".")[-3]
            transposed = leaf.startswith("deconv") or leaf.startswith("upsampled_flow")
            gain = 1.0 if (leaf.startswith("predict_flow") or leaf.startswith("upsampled_flow")) else 2.0 / 1.01
            std = float(np.sqrt(gain / _fan_in(k, shape, transposed)))
            out[k] = normal(seed, k, shape, std=std)
        elif k.endswith(".bias"):
            out[k] = uniform(seed, k, shape, -0.05, 0.05)
        elif k.endswith(".weight"):  # BN gamma (batchNorm=True variants)
            out[k] = uniform(seed, k, shape, 0.5, 1.5)
        else:
            raise KeyError(k)
    return out
