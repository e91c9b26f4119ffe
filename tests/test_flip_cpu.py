"""CPU suite of the flip test: pins the references and case tables of tests/flip_ref.py (to tools.pose.main._flip_back and to
answers known by construction), the C-ABI surface of the two new entries (exported, declared, refusing what the header forbids
without a device), DeconvResnet.flip_pairs validation, and validate()'s generic two-pass path for models without forward_flip."""
import ctypes

import numpy as np
import pytest
import torch

import flip_ref as F
import keypoint_ref as R
from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd._lib import FlowtrackHipError
from tools.pose import main as pose_main

SIZES = pytest.mark.parametrize("size", R.MAX_PREDS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _eager_flip_average(hm, hm_flip, pairs):
    """What validate()'s generic path computes from the two passes' heat maps (tools/pose/main.py)."""
    return (torch.from_numpy(np.array(hm)) + pose_main._flip_back(torch.from_numpy(np.array(hm_flip)), pairs)) * 0.5


# ---- the reference is what validate() computes today -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pairs", [("coco17_7x9", F.COCO_PAIRS), ("coco17_96x72", F.COCO_PAIRS), ("mpii16_64x48", F.MPII_PAIRS),
                                        ("k5_one_pair_8x6", ((1, 3),)), ("k1_9x1", ())])
def test_flip_merge_ref_is_validates_arithmetic(name, pairs):
    hm, hf, perm = F.perm_case(name)
    assert perm == F.perm_from_pairs(pairs, hm.shape[1])
    assert torch.equal(torch.from_numpy(F.flip_merge_ref(hm, hf, perm)), _eager_flip_average(hm, hf, pairs))


def test_pair_tables_restate_the_tools():
    assert [tuple(p) for p in pose_main.FLIP_PAIRS["coco"]] == list(F.COCO_PAIRS)
    assert [tuple(p) for p in pose_main.FLIP_PAIRS["mpii"]] == list(F.MPII_PAIRS)


def test_hflip_ref_is_torch_flip():
    for shape in F.HFLIP_SHAPES:
        x = F.hflip_input(shape)
        assert torch.equal(torch.from_numpy(F.hflip_ref(x)), torch.flip(torch.from_numpy(np.array(x)), dims=[3]))


def test_out_of_range_entries_read_as_identity():
    assert F.effective_perm((2, 7, 0), 3) == (2, 1, 0) and F.effective_perm((1, 0, -1), 3) == (1, 0, 2) and F.effective_perm(None, 2) == (0, 1)
    hm, hf, perm = F.perm_case("k3_out_of_range_17x19")
    assert np.array_equal(F.flip_merge_ref(hm, hf, perm), F.flip_merge_ref(hm, hf, (2, 1, 0)))


def test_perm_cases_show_a_wrong_channel():
    """A merged map's mean is within 0.2 of (4 (k + 1) + 100 n + 1000 + 8 (perm[k] + 1) + 300 n) / 2, and those differ by at least 2
    between any two (k, source) choices of a crop that are not the right one."""
    for name in F.PERM_CASES:
        hm, hf, perm = F.perm_case(name)
        N, K = hm.shape[:2]
        eff = F.effective_perm(perm, K)
        mean = F.flip_merge_ref(hm, hf, perm).reshape(N, K, -1).astype(np.float64).mean(axis=2)
        for n in range(N):
            for k in range(K):
                assert abs(mean[n, k] - (4 * (k + 1) + 1000 + 8 * (eff[k] + 1) + 400 * n) / 2) < 0.5, (name, n, k)


# ---- planted cases: merged == M, so every plant keeps its property --------------------------------------------------------------
@pytest.mark.parametrize("layout", R.MAX_PREDS_LAYOUTS)
@SIZES
def test_planted_cases_reproduce_the_planted_maps(size, layout):
    hm, hf, perm, names = F.planted_case(*size, layout)
    M, names_m = R.max_preds_case(*size, layout)
    assert names == names_m and np.array_equal(_bits(hm), _bits(M))
    assert np.array_equal(_bits(F.flip_merge_ref(hm, hf, perm)), _bits(M))
    if hm.shape[1] > 1:
        assert perm != tuple(range(hm.shape[1]))                 # the channel swap is really exercised
    for adjust in (0, 1):
        _, idx, rows = F.flip_keypoints_ref(hm, hf, perm, adjust)
        w_idx, w_score, w_coords = R.max_preds_ref64(M, adjust)
        assert np.array_equal(idx, w_idx) and np.array_equal(rows[..., :2], w_coords) and np.array_equal(_bits(rows[..., 2]), _bits(w_score))


@pytest.mark.parametrize("size", R.MAX_PREDS_SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nan_case_carries_the_nan_maps(size):
    hm, hf, perm, filled = F.nan_case(*size)
    merged = F.flip_merge_ref(hm, hf, perm)
    assert np.array_equal(np.isnan(merged), np.isnan(hm))
    keep = ~np.isnan(hm)
    assert np.array_equal(_bits(merged)[keep], _bits(hm)[keep]) and np.array_equal(merged[keep], filled[keep])


# ---- sum cases: each has the property it is named for ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", F.SUM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sum_cases_have_their_properties(size):
    H, W = size
    hm, hf, perm, info = F.sum_case(H, W)
    b = F.flip_merge_ref(np.zeros_like(hm), hf, perm) * np.float32(2.0)       # the mirrored pass seen in hm's frame (exact)
    merged, idx, rows = F.flip_keypoints_ref(hm, hf, perm, 1)
    a_idx, _, a_coords = R.max_preds_ref64(hm, 1)
    b_idx, _, _ = R.max_preds_ref64(b, 1)
    k = F.SUM_KINDS.index("tie_by_merge")
    p, q = info["tie_by_merge"]["p"], info["tie_by_merge"]["q"]
    flat = merged[0, k].ravel()
    assert p < q and flat[p] == flat[q] == 2.0 and (np.delete(flat, [p, q]) < 0).all()
    assert idx[0, k] == p and a_idx[0, k] == q and b_idx[0, k] == p
    k = F.SUM_KINDS.index("max_in_neither_pass")
    c = info["max_in_neither_pass"]
    assert idx[0, k] == c["c"] and a_idx[0, k] == c["pa"] and b_idx[0, k] == c["pb"] and len({c["c"], c["pa"], c["pb"]}) == 3
    k = F.SUM_KINDS.index("nudge_sign_flips")
    y, x = info["nudge_sign_flips"]["y"], info["nudge_sign_flips"]["x"]
    assert idx[0, k] == a_idx[0, k] == y * W + x
    assert a_coords[0, k].tolist() == [x - 0.25, y + 0.25] and rows[0, k, :2].tolist() == [x + 0.25, y - 0.25]
    k = F.SUM_KINDS.index("max_exactly_zero")
    z = info["max_exactly_zero"]["z"]
    assert idx[0, k] == z and _bits(rows[0, k, 2:3])[0] == 0 and rows[0, k, :2].tolist() == [0.0, 0.0]
    assert a_coords[0, k].tolist() != [0.0, 0.0]                  # pass a alone has a positive maximum there
    # adjust = 0 drops the nudge and nothing else
    _, idx0, rows0 = F.flip_keypoints_ref(hm, hf, perm, 0)
    assert np.array_equal(idx0, idx) and rows0[0, F.SUM_KINDS.index("nudge_sign_flips"), :2].tolist() == [float(x), float(y)]


# ---- library surface -------------------------------------------------------------------------------------------------------------
def test_library_exports_and_declares_the_flip_entries(hip_lib):
    for name in ("ft_hflip_nchw_f32", "ft_heatmap_flip_merge"):
        assert hasattr(hip_lib, name), f"{name} is not exported"
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._PROTOTYPES
    assert len(_lib._PROTOTYPES["ft_hflip_nchw_f32"][1]) == 7 and len(_lib._PROTOTYPES["ft_heatmap_flip_merge"][1]) == 12


def test_flip_entries_refuse_bad_arguments_without_a_device(hip_lib):
    """Statuses, not aborts, and no launch: the pointers are never dereferenced (no device is needed), as in
    tests/test_host_cpu.py::test_bad_arguments_return_status_not_abort."""
    INVALID = 1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    hflip, merge = hip_lib.ft_hflip_nchw_f32, hip_lib.ft_heatmap_flip_merge
    assert hflip(None, p, 1, 1, 1, 1, None) == INVALID and hflip(p, None, 1, 1, 1, 1, None) == INVALID
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1), (1, 1, 1, -4)):
        assert hflip(p, p, *dims, None) == INVALID, dims
    assert merge(None, p, None, 1, 1, 1, 1, 0, p, None, None, None) == INVALID
    assert merge(p, None, None, 1, 1, 1, 1, 0, p, None, None, None) == INVALID
    assert merge(p, p, None, 1, 1, 1, 1, 0, None, None, None, None) == INVALID          # all three outputs NULL
    assert merge(p, p, None, 1, 1, 1, 1, 0, p, p, None, None) == INVALID                # idx without rows
    assert merge(p, p, None, 1, 1, 1, 1, 0, p, None, p, None) == INVALID                # rows without idx
    assert merge(p, p, None, 1, 1, 1, 1, 0, None, p, None, None) == INVALID
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, -3, 1, 1)):
        assert merge(p, p, None, *dims, 0, p, p, p, None) == INVALID, dims


# ---- DeconvResnet.flip_pairs -----------------------------------------------------------------------------------------------------
def test_flip_pairs_validation():
    from flowtrack.pytorch_amd.pose import models
    m = models.deconv("resnet50", 17, False).eval()
    assert m.flip_pairs is None and m._flip_perm() is None
    m.flip_pairs = F.COCO_PAIRS
    assert m._flip_perm() == F.perm_from_pairs(F.COCO_PAIRS, 17)
    m.flip_pairs = ()
    assert m._flip_perm() == tuple(range(17))
    for bad in (((1, 2), (2, 3)), ((1, 2), (3, 1)), ((0, 17),), ((17, 0),), ((-1, 2),)):
        m.flip_pairs = bad
        with pytest.raises(FlowtrackHipError):
            m._flip_perm()
        with pytest.raises(FlowtrackHipError):
            m.plan_for(1, 64, 64)
    m.flip_pairs = None
    with pytest.raises(FlowtrackHipError, match="flip_pairs"):
        m.forward_flip(torch.zeros(1, 3, 64, 64))
    m.flip_pairs = F.COCO_PAIRS
    m.exact_in_plan = True
    with pytest.raises(FlowtrackHipError, match="flip"):
        m.plan_for(1, 64, 64)
    m.exact_in_plan = False
    m.keypoints_in_plan = True
    for call in (lambda: m.exact_submit(torch.zeros(1, 3, 64, 64)), lambda: m.forward_keypoint_rows_exact(torch.zeros(1, 3, 64, 64)),
                 lambda: m.exact_submit_plan(object())):
        with pytest.raises(FlowtrackHipError, match="flip"):
            call()


# ---- validate(): models without forward_flip keep the generic path -----------------------------------------------------------------
def test_validate_on_cpu_takes_the_generic_path():
    class StandIn(torch.nn.Module):
        """A CPU 'pose net' that counts its calls; it HAS forward_flip, which a CPU run must not use."""
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 17, 5, stride=4, padding=2)
            self.calls, self.flip_pairs = 0, "untouched"

        def forward(self, x):
            self.calls += 1
            return self.conv(x)

        def forward_flip(self, x):
            raise AssertionError("validate(device='cpu') must not call forward_flip")

    def preds_fn(hm, center, scale, adjust):
        seen.append(hm.detach().clone())
        B, K = hm.shape[:2]
        return np.zeros((B, K, 2)), np.zeros((B, K, 1))

    torch.manual_seed(0)
    net, seen = StandIn().eval(), []
    x = torch.randn(3, 3, 64, 48)
    meta = {"center": np.zeros((3, 2)), "scale": np.ones(3), "index": np.arange(3)}
    with torch.no_grad():
        pose_main.validate(net, [(x, meta)], flip_test=True, device="cpu", preds_fn=preds_fn)
        want = (net.conv(x) + pose_main._flip_back(net.conv(torch.flip(x, dims=[3])), pose_main.COCO_FLIP_PAIRS)) * 0.5
    assert net.calls == 2 and net.flip_pairs == "untouched" and torch.equal(seen[0], want)
    plain = torch.nn.Sequential(torch.nn.Conv2d(3, 17, 5, stride=4, padding=2)).eval()      # no forward_flip at all
    seen.clear()
    with torch.no_grad():
        pose_main.validate(plain, [(x, meta)], flip_test=True, device="cpu", preds_fn=preds_fn)
        want = (plain(x) + pose_main._flip_back(plain(torch.flip(x, dims=[3])), pose_main.COCO_FLIP_PAIRS)) * 0.5
    assert torch.equal(seen[0], want)
