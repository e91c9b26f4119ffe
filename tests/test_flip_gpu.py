"""The flip test on the GPU: the two kernels launched alone through the C ABI (a sentinel around every output) against the
references and case tables of tests/flip_ref.py, which tests/test_flip_cpu.py pins; then the flip plans of DeconvResnet, validate()
and PoseRunner.

EXACT (torch.equal; scores and merged values as int32 bits):
  ft_hflip_nchw_f32         against torch.flip, both paths, a second grid-stride trip of each
  ft_heatmap_flip_merge     merged, idx and rows of every case of flip_ref; merged alone (idx = rows = NULL) and idx / rows alone
                            (merged = NULL) give the same bits
  forward_flip(x)           == flip_merge_ref of the plan's own two halves (the launches are wired to the right halves); replays
  forward_keypoint_rows(x)  == ft_heatmap_keypoint_rows of the plan's own merged maps
  validate(flip_test=True)  == final_preds of the plan's merged maps
BOUNDED (bars the project already has; nothing new):
  plan.heatmaps_raw[B:] vs the model's own forward(torch.flip(x))   1e-3 max-abs (the 2B plan may pick other split-K tiles)
  fp32 merged maps vs the CPU oracle's flip average                 1e-3 max-abs (the fp32 bar of test_pose_gpu.py)
  fp16 merged maps vs the CPU oracle's flip average                 3e-3 x range of that average (test_pose_fp16_vs_fp32_oracle)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flip_ref as F
import keypoint_ref as R
from flowtrack.pytorch_amd import _lib, synth
from flowtrack.pytorch_amd._lib import FlowtrackHipError, check
from flowtrack.pytorch_amd.pose import evaluation, models
from oracle import pose_ref

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
ISENTINEL = -7
GUARD = 4                                    # elements in front of and behind every output: 16 bytes, so alignment is kept
SIZES = pytest.mark.parametrize("size", R.MAX_PREDS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
SEED = 31
PLAN_SHAPES = [(2, 64, 64), (3, 128, 96)]
SHAPES = pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(n, dtype=torch.float32):
    """(whole buffer, the n elements a call may write): the sentinel everywhere, GUARD elements on each side."""
    buf = torch.full((n + 2 * GUARD,), ISENTINEL if dtype == torch.int32 else SENTINEL, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(*bufs):
    for buf in bufs:
        fill = ISENTINEL if buf.dtype == torch.int32 else SENTINEL
        if not (bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())):
            return False
    return True


def _bits(t):
    return t.contiguous().view(torch.int32)


def _t(a):
    return torch.from_numpy(np.array(a))


# ---- ft_hflip_nchw_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.HFLIP_SHAPES + F.HFLIP_SECOND_TRIP, ids=lambda s: "x".join(str(v) for v in s[:4]) + (f"+{s[4]}B" if s[4] else ""))
def test_hflip_nchw(hip_lib, shape):
    """torch.equal with torch.flip; the (2,3,8,8) case sits 4 bytes off a 16-byte boundary on both sides (W % 4 == 0, scalar path)."""
    N, C, H, W, off = shape
    n, o = N * C * H * W, off // 4
    x = _t(F.hflip_input(shape))
    src = torch.full((n + o,), SENTINEL, dtype=torch.float32, device="cuda")
    src[o:] = x.reshape(-1).cuda()
    buf = torch.full((n + 2 * GUARD + o,), SENTINEL, dtype=torch.float32, device="cuda")
    y = buf[GUARD + o:GUARD + o + n]
    assert src.data_ptr() % 16 == 0 and y.data_ptr() % 16 == off and src[o:].data_ptr() % 16 == off
    check(hip_lib.ft_hflip_nchw_f32(src[o:].data_ptr(), y.data_ptr(), N, C, H, W, _stream()), "ft_hflip_nchw_f32")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD + o] == SENTINEL).all()) and bool((buf[GUARD + o + n:] == SENTINEL).all()), "ft_hflip_nchw_f32 wrote outside y"
    got = y.cpu().view(N, C, H, W)
    assert torch.equal(_bits(got), _bits(torch.flip(x, dims=[3]))) and torch.equal(got, _t(F.hflip_ref(x.numpy())))


# ---- ft_heatmap_flip_merge ------------------------------------------------------------------------------------------------------
def _run_merge(hip_lib, hm, hf, perm, adjust, want_merged=True, want_rows=True):
    N, K, H, W = hm.shape
    g, gf = _t(hm).cuda(), _t(hf).cuda()
    gp = torch.tensor(list(perm), dtype=torch.int32, device="cuda") if perm is not None else None
    (bm, merged), (bi, idx), (br, rows) = _out(N * K * H * W), _out(N * K, torch.int32), _out(N * K * 3)
    check(hip_lib.ft_heatmap_flip_merge(g.data_ptr(), gf.data_ptr(), gp.data_ptr() if gp is not None else None, N, K, H, W, adjust,
                                        merged.data_ptr() if want_merged else None, idx.data_ptr() if want_rows else None,
                                        rows.data_ptr() if want_rows else None, _stream()), "ft_heatmap_flip_merge")
    torch.cuda.synchronize()
    assert _guards_intact(bm, bi, br), "ft_heatmap_flip_merge wrote outside merged[N*K*H*W] / idx[N*K] / rows[N*K*3]"
    if not want_merged:
        assert bool((bm == SENTINEL).all()), "merged = NULL, and something was written"
    if not want_rows:
        assert bool((bi == ISENTINEL).all()) and bool((br == SENTINEL).all()), "idx = rows = NULL, and something was written"
    return merged.cpu().view(N, K, H, W), idx.cpu().view(N, K), rows.cpu().view(N, K, 3)


def _same_bits_nan_aware(got, want):
    """Bit for bit where `want` is a number; a NaN where it is NaN (the payload of a NaN sum is not the reference's business)."""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _check_merge(hip_lib, hm, hf, perm, adjust, want, what, names=None, maps=None):
    """All three outputs, then merged alone, then idx / rows alone: each equal to `want` = (merged, idx, rows) bit for bit.
    maps: the (n, k) maps whose key points are defined (all by default)."""
    w_merged, w_idx, w_rows = (_t(a) for a in want)
    sel = (slice(None), slice(None)) if maps is None else maps
    for want_merged, want_rows in ((True, True), (True, False), (False, True)):
        merged, idx, rows = _run_merge(hip_lib, hm, hf, perm, adjust, want_merged, want_rows)
        form = f"{what} adjust {adjust} merged {'out' if want_merged else 'NULL'} rows {'out' if want_rows else 'NULL'}"
        if want_merged:
            assert _same_bits_nan_aware(merged, w_merged), f"{form}: merged differs in {int((_bits(merged) != _bits(w_merged)).sum())} elements"
        if want_rows:
            bad = (idx != w_idx) | (_bits(rows) != _bits(w_rows)).any(dim=2)
            if maps is not None:
                keep = torch.zeros_like(bad)
                keep[sel] = True
                bad &= keep
            if bool(bad.any()):
                n, k = (int(v) for v in bad.nonzero()[0])
                name = f" '{names[n * idx.shape[1] + k]}'" if names else ""
                raise AssertionError(f"{form}: {int(bad.sum())} maps differ, first map ({n}, {k}){name}: idx {int(idx[n, k])} want {int(w_idx[n, k])}, "
                                     f"rows {rows[n, k].tolist()} want {w_rows[n, k].tolist()}")
    return merged, idx, rows


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("layout", R.MAX_PREDS_LAYOUTS)
@SIZES
def test_flip_merge_planted(hip_lib, size, layout, adjust):
    """hm = the planted maps of keypoint_ref, hm_flip = the same maps behind the mirror and a pair-swapping permutation: merged is
    the planted maps again, so every tie (one thread, lanes, waves), border maximum, nudge and the subnormal / zero scores are judged
    on the merge kernel as they are on ft_heatmap_max_preds."""
    H, W = size
    hm, hf, perm, names = F.planted_case(H, W, layout)
    want = F.flip_keypoints_ref(hm, hf, perm, adjust)
    assert np.array_equal(want[0].view(np.int32), np.array(hm).view(np.int32))
    _check_merge(hip_lib, hm, hf, perm, adjust, want, f"planted {H}x{W} {layout}", names)


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("size", F.SUM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_flip_merge_sum_cases(hip_lib, size, adjust):
    """What only the sum decides: a tie the merge creates (first pixel wins), a maximum neither pass has, a nudge whose sign the merge
    turns round, a merged maximum of exactly 0 (coordinates zeroed)."""
    hm, hf, perm, _ = F.sum_case(*size)
    _check_merge(hip_lib, hm, hf, perm, adjust, F.flip_keypoints_ref(hm, hf, perm, adjust), f"sum {size}", F.SUM_KINDS)


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("name", list(F.PERM_CASES))
def test_flip_merge_permutations(hip_lib, name, adjust):
    """COCO, MPII, one pair among fixed joints, K = 1 (with and without a perm), out-of-range entries read as identity; every map has
    a constant of its own, so a wrong channel or crop moves the merged values by >= 2."""
    hm, hf, perm = F.perm_case(name)
    _check_merge(hip_lib, hm, hf, perm, adjust, F.flip_keypoints_ref(hm, hf, perm, adjust), f"perm {name}")


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("size", R.MAX_PREDS_SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_flip_merge_never_picks_a_nan(hip_lib, size, adjust):
    """The NaN promise of ft_heatmap_keypoint_rows carries over: a NaN is never the arg-max (maps 0, 1, 3 answer as the maps with
    every NaN replaced by a very negative number), and a map of nothing but NaN gives idx 0 and coords (0, 0)."""
    hm, hf, perm, filled = F.nan_case(*size)
    w_idx, w_score, w_coords = R.max_preds_ref64(filled, adjust)
    want = (F.flip_merge_ref(hm, hf, perm), w_idx, np.concatenate((w_coords, w_score[..., None]), axis=2).astype(np.float32))
    _, idx, rows = _check_merge(hip_lib, hm, hf, perm, adjust, want, f"nan {size}", maps=(slice(None), [0, 1, 3]))
    assert int(idx[0, 2]) == 0 and rows[0, 2, :2].tolist() == [0.0, 0.0]


# ---- flip plans -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state_dict():
    return synth.fill_pose_state_dict(models.deconv("resnet50", num_classes=17, pretrained=False).state_dict(), SEED)


def _new_model(dtype):
    m = models.deconv("resnet50", num_classes=17, pretrained=False)
    m.load_state_dict(_state_dict())
    m = m.cuda().eval()
    m.compute_dtype = dtype
    return m


@functools.lru_cache(maxsize=None)
def _model(dtype):
    """One model per compute dtype for the whole module; a test sets the attributes it needs and puts them back."""
    return _new_model(dtype)


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """(x, the CPU oracle's flip average of x), computed once per shape as tests/test_tools_gpu.py does."""
    B, H, W = shape
    x = synth.pose_crops(SEED, B, H, W)
    sd = _state_dict()
    hm = pose_ref.pose_forward(sd, x)
    hf = torch.flip(pose_ref.pose_forward(sd, torch.flip(x, dims=[3])), dims=[3])
    return x, (hm + hf[:, list(F.perm_from_pairs(F.COCO_PAIRS, 17))]) * 0.5


class _attrs:
    """with _attrs(m, flip_pairs=..., keypoints_in_plan=...): set, and restore on exit."""

    def __init__(self, m, **kw):
        self.m, self.kw = m, kw

    def __enter__(self):
        self.old = {k: getattr(self.m, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.m, k, v)
        return self.m

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.m, k, v)


@SHAPES
def test_flip_plan_fp32(hip_lib, shape):
    B, H, W = shape
    x, want = _oracle(shape)
    perm = F.perm_from_pairs(F.COCO_PAIRS, 17)
    with _attrs(_model(torch.float32), flip_pairs=F.COCO_PAIRS, keypoints_in_plan=None) as m:
        got = m.forward_flip(x.cuda())
        plan = m._last_plan
        assert plan is m.plan_for(B, H, W) and tuple(plan.x_static.shape) == (B, 3, H, W) and tuple(plan.x_full.shape) == (2 * B, 3, H, W)
        assert plan.x_static.data_ptr() == plan.x_full.data_ptr() and plan.kp_rows is None and plan.kp_idx is None
        assert got.data_ptr() != plan.heatmaps.data_ptr() and tuple(got.shape) == (B, 17, H // 4, W // 4) == tuple(plan.heatmaps.shape)
        raw = plan.heatmaps_raw.cpu()
        assert tuple(raw.shape) == (2 * B, 17, H // 4, W // 4)
        assert torch.equal(plan.x_full[B:].cpu(), torch.flip(x, dims=[3])) and torch.equal(plan.x_static.cpu(), x)
        # the two launches around the trunk are wired to the right halves
        assert torch.equal(_bits(got.cpu()), _bits(_t(F.flip_merge_ref(raw[:B].numpy(), raw[B:].numpy(), perm))))
        # the second half is the net's answer to the mirrored crops
        own = m(torch.flip(x, dims=[3]).cuda()).cpu()
        err_half = (raw[B:] - own).abs().max().item()
        # against the CPU oracle's flip average, and a replay
        err = (got.cpu() - want).abs().max().item()
        print(f"flip plan fp32 {shape}: second half vs own forward {err_half:.3e}, merged vs oracle {err:.3e}")
        assert err_half <= 1e-3 and err <= 1e-3
        again = m.forward_flip(x.cuda())
        assert plan.runs >= 2 and torch.equal(_bits(again), _bits(got))
        assert torch.equal(_bits(m.forward_flip(x.cuda(), copy_output=False)), _bits(got))
        # forward() keeps returning the heat maps of x and never reads flip_pairs
        plain = m(x.cuda()).cpu()
        assert (plain - raw[:B]).abs().max().item() <= 1e-3 and not torch.equal(plain, got.cpu())


@SHAPES
def test_flip_plan_fp16(hip_lib, shape):
    """The bar of test_pose_fp16_vs_fp32_oracle on the oracle's flip average (no new tolerance: the average of two maps that each meet
    the bar meets it; the range is taken of the average itself, which is never wider than the two maps').
    Measured on an MI355X: 2 x 64x64 max-abs 1.039e-03 on a range of 2.168 = 0.160 of the bar; 3 x 128x96 1.544e-03 on 3.424 = 0.150."""
    B, H, W = shape
    x, want = _oracle(shape)
    with _attrs(_model(torch.float16), flip_pairs=F.COCO_PAIRS, keypoints_in_plan=None) as m:
        got = m.forward_flip(x.cuda()).cpu()
        raw = m._last_plan.heatmaps_raw.cpu()
        assert torch.equal(_bits(got), _bits(_t(F.flip_merge_ref(raw[:B].numpy(), raw[B:].numpy(), F.perm_from_pairs(F.COCO_PAIRS, 17)))))
        err = (got - want).abs().max().item()
        rng = (want.max() - want.min()).item()
        print(f"flip plan fp16 {shape}: merged vs oracle {err:.3e}, range {rng:.3f}, err / (3e-3 range) = {err / (3e-3 * rng):.3f}")
        assert err <= 3e-3 * rng, f"fp16 flip-averaged heatmap error {err:.3e} vs range {rng:.2f}"
        assert torch.equal(_bits(m.forward_flip(x.cuda()).cpu()), _bits(got))


@pytest.mark.parametrize("adjust", [True, False])
def test_flip_plan_keypoint_rows(hip_lib, adjust):
    """With keypoints_in_plan the merge launch writes the rows: those of ft_heatmap_keypoint_rows on the plan's own merged maps."""
    shape = PLAN_SHAPES[0]
    B, H, W = shape
    x, _ = _oracle(shape)
    with _attrs(_model(torch.float32), flip_pairs=F.COCO_PAIRS, keypoints_in_plan=adjust) as m:
        rows = m.forward_keypoint_rows(x.cuda())
        plan = m._last_plan
        assert rows.data_ptr() == plan.kp_rows.data_ptr() and hasattr(plan, "heatmaps_raw") and not any(c[0] == "ft_heatmap_keypoint_rows" for c in plan.prog.calls)
        hm = plan.heatmaps
        (bi, idx), (br, want) = _out(B * 17, torch.int32), _out(B * 17 * 3)
        check(hip_lib.ft_heatmap_keypoint_rows(hm.data_ptr(), B, 17, hm.shape[2], hm.shape[3], int(adjust), idx.data_ptr(), want.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(_bits(rows.reshape(-1)), _bits(want)) and torch.equal(plan.kp_idx.reshape(-1), idx)
        raw = plan.heatmaps_raw.cpu().numpy()
        _, r_idx, r_rows = F.flip_keypoints_ref(raw[:B], raw[B:], F.perm_from_pairs(F.COCO_PAIRS, 17), int(adjust))
        assert torch.equal(_bits(rows.cpu()), _bits(_t(r_rows))) and torch.equal(plan.kp_idx.cpu(), _t(r_idx))
        hm2, idx2, score2, coords2 = m.forward_keypoints(x.cuda())
        assert hm2.data_ptr() == hm.data_ptr() and torch.equal(score2, rows[:, :, 2:]) and torch.equal(coords2, rows[:, :, :2])


def test_flip_pairs_none_changes_nothing(hip_lib):
    shape = PLAN_SHAPES[0]
    B, H, W = shape
    x, _ = _oracle(shape)
    fresh = _new_model(torch.float32)                      # flip_pairs never touched
    assert "flip_pairs" not in fresh.__dict__ and fresh.flip_pairs is None
    hm = fresh(x.cuda())
    dev = next(fresh.parameters()).device
    assert list(fresh._plans) == [(B, H, W, dev, torch.float32, None)]          # the key of a plain plan, as it always was
    fresh.keypoints_in_plan = True
    fresh.plan_for(B, H, W, replica=2)
    assert list(fresh._plans)[1] == (B, H, W, dev, torch.float32, True, 2)
    with _attrs(_model(torch.float32), flip_pairs=F.COCO_PAIRS, keypoints_in_plan=None) as m:
        assert torch.equal(_bits(m(x.cuda())), _bits(hm))                       # forward() with flip_pairs set: the same plain plan
        assert (B, H, W, dev, torch.float32, None) in m._plans
    with _attrs(_model(torch.float32), flip_pairs=None) as m:
        assert torch.equal(_bits(m(x.cuda())), _bits(hm))
        with pytest.raises(FlowtrackHipError, match="flip_pairs"):
            m.forward_flip(x.cuda())
    with _attrs(fresh, flip_pairs=(), keypoints_in_plan=None):                # an empty tuple is valid: mirror and average, no swap
        got = fresh.forward_flip(x.cuda()).cpu()
        raw = fresh._last_plan.heatmaps_raw.cpu().numpy()
        assert torch.equal(_bits(got), _bits(_t(F.flip_merge_ref(raw[:B], raw[B:], None))))
    fresh.close()


def test_flip_pairs_with_the_exact_mode_raises(hip_lib):
    x = _oracle(PLAN_SHAPES[0])[0].cuda()
    with _attrs(_model(torch.float16), flip_pairs=F.COCO_PAIRS, keypoints_in_plan=True, exact_in_plan=True) as m:
        for call in (lambda: m.plan_for(2, 64, 64), lambda: m.forward_flip(x), lambda: m.forward_keypoint_rows(x)):
            with pytest.raises(FlowtrackHipError, match="flip"):
                call()
    with _attrs(_model(torch.float16), flip_pairs=F.COCO_PAIRS, keypoints_in_plan=True) as m:
        for call in (lambda: m.exact_submit(x), lambda: m.forward_keypoint_rows_exact(x), lambda: m.exact_submit_plan(m.plan_for(2, 64, 64))):
            with pytest.raises(FlowtrackHipError, match="flip"):
                call()


def test_validate_uses_the_flip_plan(hip_lib):
    from tools.pose import main as pose_main
    shape = PLAN_SHAPES[0]
    B, H, W = shape
    x, _ = _oracle(shape)
    meta = {"center": np.array([[W / 2.0 + 3 * i, H / 2.0 + 2 * i] for i in range(B)]), "scale": np.full(B, H * 1.25), "index": np.arange(B)}
    m = _model(torch.float32)
    with _attrs(m, flip_pairs=((1, 2),), keypoints_in_plan=None):
        out = pose_main.validate(m, [(x, meta)], flip_test=True, flip_pairs=pose_main.COCO_FLIP_PAIRS)
        assert m.flip_pairs == ((1, 2),)                                       # restored
        m.flip_pairs = F.COCO_PAIRS
        plan = m.plan_for(B, H, W)
        assert plan.runs >= 1 and hasattr(plan, "heatmaps_raw")                # validate() ran this plan
        assert torch.equal(plan.x_static.cpu(), x)
        preds, scores = evaluation.final_preds(plan.heatmaps, meta["center"], meta["scale"], True)
        assert np.array_equal(out["preds"], np.asarray(preds, np.float64)) and np.array_equal(out["scores"], np.asarray(scores, np.float32))
        assert out["preds"].shape == (B, 17, 2)


def test_pose_runner_with_flip_pairs(hip_lib):
    from flowtrack.pytorch_amd.tracking import PoseRunner, net_utils
    from tools.pose.main import COCO_FLIP_PAIRS
    net = _model(torch.float32)
    with _attrs(net, flip_pairs=None, keypoints_in_plan=None):
        dev = next(net.parameters()).device
        frame = torch.from_numpy((synth.uniform01(6, "flip.frame", (96, 128, 3)) * 255).astype(np.uint8)).to(dev)
        boxes = np.array([[10, 12, 60, 80], [40, 5, 110, 90], [70, 30, 120, 70]], dtype=np.float64)
        runner = PoseRunner(net, inp_res=(64, 64), flip_pairs=COCO_FLIP_PAIRS)
        assert net.flip_pairs == tuple(tuple(p) for p in COCO_FLIP_PAIRS) and net.keypoints_in_plan is True
        got = runner(frame, boxes)
        plan = net.plan_for(4, 64, 64)                                          # three boxes: bucket 4
        assert plan.runs == 1 and tuple(plan.x_full.shape) == (8, 3, 64, 64) and plan.x_static.data_ptr() == net.static_input(4, 64, 64).data_ptr()
        crops, rows = plan.x_static.clone(), plan.kp_rows.clone()
        assert torch.equal(plan.x_full[4:], torch.flip(crops, dims=[3]))
        centers, scales = net_utils.boxes_to_center_scale(boxes, (64, 64))
        assert np.array_equal(got, net_utils.heatmap_rows_to_image(rows[:3].cpu().numpy(), centers, scales, (16, 16)))
        assert torch.equal(_bits(net.forward_keypoint_rows(crops)), _bits(rows))
        raw = plan.heatmaps_raw.cpu().numpy()
        _, _, r_rows = F.flip_keypoints_ref(raw[:4], raw[4:], F.perm_from_pairs(F.COCO_PAIRS, 17), 1)
        assert torch.equal(_bits(rows.cpu()), _bits(_t(r_rows)))
        runner.close()
