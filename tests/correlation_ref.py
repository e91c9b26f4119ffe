"""Float64 reference of the in-network correlation (ft_correlation_nhwc_fwd: NHWC features, kernel 1, stride1 1, pad = max
displacement) and the error bound its kernels are held to.  CPU only: a thin wrapper around flow_grad_ref.correlation_fwd."""
import torch

from flow_grad_ref import correlation_fwd

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2      # FT_ACT_*


def activation(v, act, slope):
    """act(v) = v > 0 ? v : k * v in the precision of `v`, with torch's values for NaN / +-inf (ReLU(-inf) = 0, ReLU(NaN) = NaN)."""
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    return v


def correlation_nhwc_ref(f1, f2, C, max_disp, stride2, act, slope):
    """f1, f2: NHWC tensors [B, H, W, >= C] (fp16 or fp32 values; a channel slice of a wider tensor is fine).  Returns
    (want, S), both float64 [B, H, W, D*D]: want = act(1/C sum_c a_c b_c) and S = 1/C sum_c |a_c b_c|, the scale of the
    accumulation error of that cell."""
    a = f1[..., :C].to(torch.float64).permute(0, 3, 1, 2).contiguous()
    b = f2[..., :C].to(torch.float64).permute(0, 3, 1, 2).contiguous()
    raw = correlation_fwd(a, b, pad=max_disp, k=1, md=max_disp, s1=1, s2=stride2)
    S = correlation_fwd(a.abs(), b.abs(), pad=max_disp, k=1, md=max_disp, s1=1, s2=stride2)
    want = activation(raw, act, slope)
    return want.permute(0, 2, 3, 1).contiguous(), S.permute(0, 2, 3, 1).contiguous()


def error_bound(want, S, C, fp16_out):
    """Per-element bound on |kernel - want| before the factor 2 the tests allow for the undocumented summation order of MFMA:
    C * 2^-24 * S    worst-case fp32 accumulation of C products (exact for fp16 operands),
    2^-23 * |want|   the 1/C and slope multiplies,
    and for an fp16 output 2^-11 * |want| + 2^-25: one rounding to fp16, half the subnormal spacing."""
    bound = C * 2.0 ** -24 * S + 2.0 ** -23 * want.abs()
    if fp16_out:
        bound = bound + 2.0 ** -11 * want.abs() + 2.0 ** -25
    return bound


def worst_ratio(err, bound):
    """max err / bound (float64 tensors); a cell with bound 0 (fp32 output, every product zero) has to be exact."""
    if err.numel() == 0:
        return 0.0
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(ratio.max())


def in_image_mask(H, W, max_disp, stride2):
    """bool [H, W, D*D]: True where the displaced f2 pixel of that cell lies inside the image."""
    drad = max_disp // stride2
    d = stride2 * torch.arange(-drad, drad + 1)
    y2 = torch.arange(H).view(H, 1, 1, 1) + d.view(1, 1, -1, 1)
    x2 = torch.arange(W).view(1, W, 1, 1) + d.view(1, 1, 1, -1)
    ok = (y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W)
    return ok.reshape(H, W, -1)
