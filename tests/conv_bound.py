"""The derived per-element error bound of an fp16 conv layer with fp32 accumulation, shared by the float64 parity tests of the direct
conv forms (deconv_direct_cases.py, direct_bound_cases.py)."""


def derived_bound(K, S, pre, scale, want, extra=()):
    """Per element, for a layer  want = act(pre * scale + shift (+ residual))  with pre = the sum of K exact fp16 x fp16 products and
    S = the sum of their magnitudes:
      * worst-case fp32 accumulation (every partial sum is at most S, one rounding of 2^-24 relative per add), doubled for the
        summation order inside an MFMA, plus the rounding of the sum into the scale / shift FMA:  2 (K 2^-24 S + 2^-23 |pre|) |scale|;
      * one 2^-24-relative term for every further fp32 operation of the epilogue (`extra`: the magnitudes of their results: the
        residual add, the leaky multiply);
      * one rounding to fp16: 2^-11 |want|, and 2^-25 absolute in the subnormal range."""
    b = 2.0 * (K * 2.0 ** -24 * S + 2.0 ** -23 * pre.abs()) * scale.abs().view(1, -1, 1, 1)
    for m in extra:
        b = b + 2.0 ** -24 * m.abs()
    return b + 2.0 ** -11 * want.abs() + 2.0 ** -25
