"""The derived error bound of test_conv_direct_bound_gpu.py, checked on the CPU for every case: a plain sequential fp32 evaluation of
the layer stays inside 1 x the bound, and deliberately degraded evaluations leave it — the scale table rounded to fp16, each
64-channel partial sum rounded to fp16 before it is added, truncation in place of round-to-nearest at the end.

What the bound can and cannot see follows from its own terms.  Its accumulation term is 2 K 2^-24 S |scale| per element, and S >= |pre|.
The scale table in fp16 and the partial sums in fp16 each change an element by at most 2^-11 S |scale|, so from K = 4096 on
(K 2^-23 >= 2^-11: the 3x3 forms on 512 and 1024 channels) NO data can push them outside: there the two ratios are printed and only
required to stay inside, which is the proof restated; truncation (up to 2^-10 |want| against the 2^-11 |want| of the rounding term) is
required to leave the bound in every case.  Below K = 4096 all three must leave it.

Also: deconv_direct_cases.bound, now a call of the shared conv_bound.derived_bound, returns the values of its former expression."""
import pytest
import torch

import deconv_direct_cases as deconv
import direct_bound_cases as dc


def _ratio(r, chans, mode):
    got, rows = dc.evaluate(r, chans, mode)
    return ((got - dc.rows_of(r["want"], chans, rows)).abs() / dc.rows_of(r["bound"], chans, rows)).max().item()


@pytest.mark.parametrize("name", dc.NAMES)
def test_sequential_fp32_is_inside_and_degraded_evaluations_are_outside(name):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    r = dc.reference(name)
    chans = dc.channel_subset(r["want"].shape[1])
    plain, scale16, chunk16, trunc = (_ratio(r, chans, m) for m in ("plain", "scale16", "chunk16", "truncate"))
    print(f"{name}: K = {r['K']}; max |err| / bound: sequential fp32 {plain:.3f}; scale table in fp16 {scale16:.3f}, 64-channel partial sums in "
          f"fp16 {chunk16:.3f}, truncation {trunc:.3f}")
    assert plain <= 1.0, f"{name}: a plain sequential fp32 evaluation is outside the bound ({plain:.3f})"
    assert trunc > 1.0, f"{name}: truncation stays inside the bound ({trunc:.3f}): the data is too tame"
    if r["K"] * 2.0 ** -23 < 2.0 ** -11:
        assert scale16 > 1.0, f"{name}: an fp16 scale table stays inside the bound ({scale16:.3f}): the data is too tame"
        assert chunk16 > 1.0, f"{name}: fp16 partial sums stay inside the bound ({chunk16:.3f}): the data is too tame"
    else:
        assert scale16 <= 1.0 and chunk16 <= 1.0, "2^-11 S |scale| cannot exceed K 2^-23 S |scale| from K = 4096 on"


def test_truncation_helper():
    import numpy as np
    v = np.array([1.0009765625 + 2.0 ** -12, -(1.0009765625 + 2.0 ** -12), 3.0, 65504.0, 1e-7], dtype=np.float32)
    t = dc.truncate_to_fp16(v).astype(np.float64)
    assert t.tolist()[:4] == [1.0009765625, -1.0009765625, 3.0, 65504.0] and 0.0 <= t[4] <= 1e-7


@pytest.mark.parametrize("name", deconv.IDS)
def test_deconv_bound_keeps_its_values(name):
    """The six transposed cases: the shared function gives exactly what the former expression of deconv_direct_cases.bound gave."""
    r = deconv.reference(name)
    Cin = r["x"].shape[1]
    S, pre, scale, want = r["S"], r["pre"], r["scale"], r["want"]
    former = 2.0 * (4 * Cin * 2.0 ** -24 * S + 2.0 ** -23 * pre.abs()) * scale.abs().view(1, -1, 1, 1) + 2.0 ** -11 * want.abs() + 2.0 ** -25
    assert torch.equal(deconv.bound(Cin, S, pre, scale, want), former) and torch.equal(r["bound"], former)
