"""References of the lateral-deconv pose head (lib/pose/models/pose_net.py:9-14,23-28,30-67), shared by tests/test_posenet_cpu.py,
test_deconv_lateral_gpu.py, test_posenet_gpu.py and tests/golden/make_posenet_golden.py.

  posenet_forward     torch-CPU fp32 functional restatement of PoseResnet.forward, one torch.nn.functional call per op of the reference
                      (trunk blocks from oracle/pose_ref.py); pinned against the imported reference by make_posenet_golden.py.
  pack_taps_w2        numpy restatement of the packed weights of one top-down step (include/flowtrack_hip.h, K-concat behind the
                      transposed conv): per output-parity phase the four taps of the ConvTranspose2d(4,2,1) and, behind them, the
                      1x1 lateral conv's block.
  packed_step_ref     that packed matrix multiplied out on the CPU: out[2q+p] = sum over taps of W[tap] x[q + p - t] + W2 x2[2q+p].
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pose_ref


def _bn_relu(sd, p, x):
    """The front of _make_deconv / _make_conv (pose_net.py:9-14,23-28): BatchNorm (eval) -> ReLU."""
    return F.relu(pose_ref._bn(sd, p + ".0", x))


@torch.no_grad()
def posenet_forward(sd, x, depth=50, return_features=False):
    """sd: state_dict of pose('resnet<depth>', K) (CPU tensors); x [B,3,H,W] -> heat maps [B,K,H/4,W/4] fp32 (pose_net.py:50-67)."""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    x = x.float()
    x = F.relu(pose_ref._bn(sd, "bn1", F.conv2d(x, sd["conv1.weight"], stride=2, padding=3)))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    c = []
    for li, nblocks in enumerate(pose_ref.RESNET_LAYERS[depth], start=1):
        for bi in range(nblocks):
            x = pose_ref._bottleneck(sd, f"layer{li}.{bi}", x, 2 if (bi == 0 and li > 1) else 1)
        c.append(x)
    c2, c3, c4, c5 = c

    def step(name, p, lat, cmap):
        return F.conv_transpose2d(_bn_relu(sd, name, p), sd[name + ".2.weight"], stride=2, padding=1) + F.conv2d(cmap, sd[lat + ".weight"])
    p4 = step("deconv1", c5, "latlayer2", c4)
    p3 = step("deconv2", p4, "latlayer3", c3)
    p2 = step("deconv3", p3, "latlayer4", c2)
    out = F.conv2d(_bn_relu(sd, "heatmap", p2), sd["heatmap.2.weight"], sd["heatmap.2.bias"])
    feats = {"layer1": c2, "layer2": c3, "layer3": c4, "layer4": c5, "p4": p4, "p3": p3, "p2": p2}
    return (out, feats) if return_features else out


# ---- one top-down step's packed weights ------------------------------------------------------------------------------------------
def tap_source(phase: int, tap: int):
    """(ky, kx) of ConvTranspose2d(4,2,1)'s kernel behind tap `tap` of output-parity phase `phase` = 2 py + px, the rule of
    ft_conv_tap_source: out[2q + p] takes in[q + p - t] * W[k], k = 1 + 2t for p = 0 and 2t for p = 1, per axis."""
    py, px, ty, tx = phase >> 1, phase & 1, tap >> 1, tap & 1
    return (1 + 2 * ty if py == 0 else 2 * ty), (1 + 2 * tx if px == 0 else 2 * tx)


def pack_taps_w2(wt: np.ndarray, w2: np.ndarray, cin_pad: int, cin2_pad: int, cout_pad: int) -> np.ndarray:
    """wt [Cin, Cout, 4, 4] (ConvTranspose2d layout), w2 [Cout, Cin2, 1, 1] -> [4, cout_pad, 4 cin_pad + cin2_pad]:
    k = tap * cin_pad + ci for the taps, 4 cin_pad + c2 for the lateral block (the same block in every phase), zeros in all padding."""
    cin, cout = wt.shape[:2]
    cin2 = w2.shape[1]
    out = np.zeros((4, cout_pad, 4 * cin_pad + cin2_pad), dtype=wt.dtype)
    for ph in range(4):
        for t in range(4):
            ky, kx = tap_source(ph, t)
            out[ph, :cout, t * cin_pad:t * cin_pad + cin] = wt[:, :, ky, kx].T
        out[ph, :cout, 4 * cin_pad:4 * cin_pad + cin2] = w2[:, :, 0, 0]
    return out


def packed_step_ref(packed: np.ndarray, x: np.ndarray, x2: np.ndarray, cin_pad: int, cout: int) -> np.ndarray:
    """The GEMM the kernel runs, in numpy: x [N,Cin,Hi,Wi], x2 [N,Cin2,2Hi,2Wi] -> [N,cout,2Hi,2Wi].  Row (n, qy, qx) of phase
    (py, px) is [x[n, :, qy + py - ty, qx + px - tx] for the four taps (zeros out of range) | x2[n, :, 2qy + py, 2qx + px]]."""
    N, cin, hi, wi = x.shape
    cin2 = x2.shape[1]
    y = np.zeros((N, cout, 2 * hi, 2 * wi), dtype=np.result_type(packed.dtype, x.dtype))
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        for n in range(N):
            for qy in range(hi):
                for qx in range(wi):
                    row = np.zeros(packed.shape[2], dtype=y.dtype)
                    for t in range(4):
                        iy, ix = qy + py - (t >> 1), qx + px - (t & 1)
                        if 0 <= iy < hi and 0 <= ix < wi:
                            row[t * cin_pad:t * cin_pad + cin] = x[n, :, iy, ix]
                    row[4 * cin_pad:4 * cin_pad + cin2] = x2[n, :, 2 * qy + py, 2 * qx + px]
                    y[n, :, 2 * qy + py, 2 * qx + px] = packed[ph, :cout] @ row
    return y
