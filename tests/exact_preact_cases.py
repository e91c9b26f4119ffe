"""Integer-exact data for ft_preact_conv1x1_fwd, in the style of exact_cases.py: every intermediate of the contract is exactly
representable, so a correct kernel returns the integer arithmetic's result bit for bit, whatever its summation order.

  x in -4 .. 4, pre_scale in +-{0.5, 1, 2}, pre_shift a half-integer in -4 .. 4  ->  v = fma(s, x, b) is a multiple of 0.5, |v| <= 12:
      exact in fp16 and fp32, fused or not;  r = relu(v);  pooled: the sum of four is a multiple of 0.5 up to 48, times 0.25 a
      multiple of 1/8 up to 12 (8 bits: exact in fp16)
  w in -2 .. 2  ->  a product is a multiple of 1/8 up to 24, a sum over K <= 1024 channels one up to 24576: 18 bits, exact in fp32
  post_scale in +-{0.5, 1, 2}, post_shift a half-integer  ->  a multiple of 1/16 below 2^16: 20 bits, exact in fp32
  the store rounds once to the output type: numpy's astype from the exact float64 value is that rounding (fp16: |y| < 65504 holds)
"""
import torch

from flowtrack.pytorch_amd import synth

_POW = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])


def _pick(seed, name, n):
    return _POW[torch.clamp((synth.uniform(seed, name, (n,)) * 6).long(), max=5)].double()


def exact_case(name, N, H, W, cin, cout, pool, seed=61):
    tag = f"preact.exact.{name}.{N}.{H}.{W}.{cin}.{cout}.{int(pool)}"
    return {
        "x": (torch.floor(synth.uniform(seed, tag + ".x", (N, H, W, cin)) * 9) - 4).double(),
        "w": (torch.floor(synth.uniform(seed, tag + ".w", (cout, cin)) * 5) - 2).double(),
        "pre_scale": _pick(seed, tag + ".ps", cin),
        "pre_shift": (torch.floor(synth.uniform(seed, tag + ".pb", (cin,)) * 17) - 8).double() / 2,
        "post_scale": _pick(seed, tag + ".qs", cout),
        "post_shift": (torch.floor(synth.uniform(seed, tag + ".qb", (cout,)) * 17) - 8).double() / 2,
    }


def exact_want(c, pool, relu):
    """The contract on the case's data, pixel by pixel in float64 (every step exact) -> [N, Ho, Wo, Cout] before the store's rounding."""
    r = torch.clamp(c["x"] * c["pre_scale"] + c["pre_shift"], min=0.0)
    if pool:
        N, H, W, C = r.shape
        Ho, Wo = H // 2, W // 2
        a = torch.zeros((N, Ho, Wo, C), dtype=torch.float64)
        for oy in range(Ho):
            for ox in range(Wo):
                a[:, oy, ox] = 0.25 * ((r[:, 2 * oy, 2 * ox] + r[:, 2 * oy, 2 * ox + 1]) + (r[:, 2 * oy + 1, 2 * ox] + r[:, 2 * oy + 1, 2 * ox + 1]))
        r = a
    y = torch.einsum("nhwc,oc->nhwo", r, c["w"]) * c["post_scale"] + c["post_shift"]
    return torch.clamp(y, min=0.0) if relu else y
