"""The stacked-hourglass pose model (hourglass.py:127-231): HourglassNet and its parameter layout."""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from ..hip_ops import FlowtrackHipError, fold_scale_shift, new_act, new_rowpacked_act, record_hourglass_down, record_hourglass_up, record_pack_input, record_scale_shift_act
from ..params import ActMarker, BatchNormParams, ConvParams
from .host import PoseHost, _Stages


class HgBottleneck(nn.Module):
    """Parameter layout of the hourglass's pre-activation block (hourglass.py:10-45): out = branch(relu(bn(x))) + shortcut(x) with
    branch = 1x1 -> bn -> relu -> 3x3 -> bn -> relu -> 1x1 at half the output's planes; `shortcut` is a 1x1 conv where the channel
    count changes, and the 'no_preact' form (res1, behind the stem's own ReLU) has no `preact`."""

    def __init__(self, inplanes: int, outplanes: int, preact: bool = True, bias: bool = True):
        super().__init__()
        planes = outplanes // 2
        self.shortcut = ConvParams(inplanes, outplanes, 1, bias=bias) if inplanes != outplanes else None
        if preact:
            self.preact = nn.Sequential(BatchNormParams(inplanes), ActMarker("relu"))
        self.branch = nn.Sequential(ConvParams(inplanes, planes, 1, bias=bias), BatchNormParams(planes), ActMarker("relu"),
                                    ConvParams(planes, planes, 3, padding=1, bias=bias), BatchNormParams(planes), ActMarker("relu"),
                                    ConvParams(planes, outplanes, 1, bias=bias))


def _hg_residual(inplanes: int, outplanes: int, num_blocks: int, preact: bool = True) -> nn.Sequential:
    """_make_residual (hourglass.py:56-63,175-182): num_blocks blocks, the first one carries the change of width."""
    return nn.Sequential(HgBottleneck(inplanes, outplanes, preact), *[HgBottleneck(outplanes, outplanes) for _ in range(1, num_blocks)])


class Hourglass(nn.Module):
    """Parameter layout of one hourglass (hourglass.py:47-74): hg[d] = the three chains of level d + 1 (up, low1, low3), and a
    fourth (low2) at the lowest level d = 0."""

    def __init__(self, num_blocks: int, planes: int, depth: int):
        super().__init__()
        self.depth = depth
        self.maxpool = ActMarker("maxpool2x2s2")
        self.hg = nn.ModuleList(nn.ModuleList(_hg_residual(planes, planes, num_blocks) for _ in range(4 if d == 0 else 3))
                                for d in range(depth))


class HourglassNet(PoseHost):
    """The stacked hourglass (hourglass.py:127-231; Newell et al., ECCV 2016) on the HIP path.

        x = res3(res2(maxpool(res1(pre(input)))))                                            [B, H/4, W/4, 256]
        per stack i:  y = proj[i](res[i](hg[i](x)));  heatmap_i = heatmap[i](y);  x = x + proj_[i](y) + heatmap_[i](heatmap_i)
        hg level n:   up1 = hg[n-1][0](x);  low1 = hg[n-1][1](maxpool(x));  low2 = level n-1 (low1), or hg[0][3](low1) at n = 1
                      out = up1 + upsample_ac(hg[n-1][2](low2), size of up1)

    Every block is pre-activation: conv1 reads relu(bn(x)), the residual add reads x.  A block is three conv launches — 1x1 + bn +
    relu, 3x3 + bn + relu, 1x1 + bias + residual (no activation) — and its activated input comes from where its raw input is made:
      ft_hourglass_down_fwd  at the top of every level reads the level's input once and writes a_full (for hg[n-1][0]), the pooled
                             map and its activated copy (for hg[n-1][1]); behind res1 it writes the pooled pair only;
      ft_hourglass_up_fwd    at the end of every level writes the sum (in place of up1) and its activated copy for the next block
                             (hg[n][2] of the level above, res[i] at the top);
      ft_scale_shift_act_nhwc_fwd  only where the input is a conv3 output: inside chains of more than one block, hg[0][3], the
                             lowest hg[0][2], res3.
    fuse_seams = False records the same arithmetic unfused (pool alone, sum alone, stand-alone activations): the fused outputs
    are bit-identical to it (tests/test_hourglass_gpu.py).  The join between stacks is two convs chained through the residual
    input; stack i's heat map is written twice by the same layer, NCHW fp32 for the caller and NHWC as heatmap_[i]'s input."""
    #: write the activated copies at the level seams (ft_hourglass_down_fwd / ft_hourglass_up_fwd) instead of stand-alone launches
    fuse_seams: bool = True
    depth, num_feats = 4, 256
    zero_conv_bias = True       # hourglass.py:166-173; the init is the constructor's, there is no init_net in the reference

    def __init__(self, num_classes: int, num_stacks: int, num_blocks: int):
        super().__init__()
        self.num_classes, self.num_stacks, self.num_blocks = num_classes, num_stacks, num_blocks
        feats = self.num_feats
        self.pre = nn.Sequential(ConvParams(3, 64, 7, stride=2, padding=3, bias=True), BatchNormParams(64), ActMarker("relu"))
        self.res1 = _hg_residual(64, 256, 1, preact=False)
        self.res2 = _hg_residual(256, 256, 1)
        self.res3 = _hg_residual(256, feats, 1)
        self.maxpool = ActMarker("maxpool2x2s2")
        self.hg = nn.ModuleList(Hourglass(num_blocks, feats, self.depth) for _ in range(num_stacks))
        self.res = nn.ModuleList(_hg_residual(feats, feats, num_blocks) for _ in range(num_stacks))
        self.proj = nn.ModuleList(nn.Sequential(ConvParams(feats, feats, 1), BatchNormParams(feats), ActMarker("relu")) for _ in range(num_stacks))
        self.heatmap = nn.ModuleList(ConvParams(feats, num_classes, 1) for _ in range(num_stacks))
        self.proj_ = nn.ModuleList(ConvParams(feats, feats, 1) for _ in range(num_stacks - 1))
        self.heatmap_ = nn.ModuleList(ConvParams(num_classes, feats, 1) for _ in range(num_stacks - 1))
        self.init_weights()

    def _check_input_size(self, H: int, W: int) -> None:
        low = 1 << self.depth
        if H % 4 or W % 4 or H // 4 < low or W // 4 < low:
            raise FlowtrackHipError(f"input {H}x{W}: height and width must be multiples of 4 and at least {4 * low} (the map of the "
                                    f"hourglass's lowest level, 1/{4 * low} of the input rounded down, must not be empty)")

    @torch.no_grad()
    def forward(self, x: torch.Tensor, copy_output: bool = True) -> List[torch.Tensor]:
        """x: [B,3,H,W] on the model's GPU -> the reference's list of num_stacks heat-map tensors [B,K,H/4,W/4] fp32, one per
        stack (hourglass.py:203-225); the last one is what plans, the flip test and the key points are built on."""
        self._forward(x, False, None)
        maps = [self._last_plan.stages[f"heatmap.{i}"] for i in range(self.num_stacks)]
        return [t.clone() for t in maps] if copy_output else maps

    # -- the launch list --------------------------------------------------------------------------------------------------------
    def _bn_table(self, name: str, bn, dtype, device):
        """(scale, shift) fp32 [C] of an eval-mode BatchNorm for the element-wise kernels, folded once per (dtype, device)."""
        return self._cached(name + ".scale_shift", dtype, device, lambda: fold_scale_shift(bn.num_features, bn.num_features, None, bn.as_dict(), device))

    def _record_net(self, prog, x_static, dtype, device):
        B, _, H, W = x_static.shape
        mk = dict(dtype=dtype, device=device)
        stages = _Stages()
        scratch = {}

        def tmp(tag, h, w, c):          # t1 / t2 of a block: read by the next launch only, so one buffer per size serves every block
            key = (tag, h, w, c)
            if key not in scratch:
                scratch[key] = new_act(B, h, w, c, dtype, device)
            return scratch[key]

        def act_of(name, blk, raw):     # stand-alone relu(bn(raw)) for block `name`
            a = new_act(B, raw.H, raw.W, raw.C, dtype, device)
            record_scale_shift_act(prog, raw, a, *self._bn_table(name + ".preact.0", blk.preact[0], dtype, device), "relu")
            return a

        def block(name, blk, raw, a):
            br = blk.branch
            c1 = self.fused(name + ".branch.0", br[0].weight, bias=br[0].bias, bn=br[1].as_dict(), act="relu", **mk)
            c2 = self.fused(name + ".branch.3", br[3].weight, pad=1, bias=br[3].bias, bn=br[4].as_dict(), act="relu", **mk)
            c3 = self.fused(name + ".branch.6", br[6].weight, bias=br[6].bias, act=None, **mk)
            t1, t2 = tmp("t1", raw.H, raw.W, c1.cout), tmp("t2", raw.H, raw.W, c2.cout)
            c1.record(prog, a, t1)
            c2.record(prog, t1, t2)
            res = raw
            if blk.shortcut is not None:        # res1's 64 -> 256 projection: a conv of its own that feeds the residual input
                res = new_act(B, raw.H, raw.W, c3.cout, dtype, device)
                self.fused(name + ".shortcut", blk.shortcut.weight, bias=blk.shortcut.bias, act=None, **mk).record(prog, raw, res)
            out = new_act(B, raw.H, raw.W, c3.cout, dtype, device)
            c3.record(prog, t2, out, residual=res)
            return out

        def chain(name, seq, raw, a):   # a = the first block's activated input where a seam wrote it, else None
            for k, blk in enumerate(seq):
                bname = f"{name}.{k}"
                if a is None:
                    a = act_of(bname, blk, raw)
                raw, a = block(bname, blk, raw, a), None
            return raw

        def down(x, tab_pool, tab_full):
            pool = new_act(B, x.H // 2, x.W // 2, x.C, dtype, device)
            a_pool = new_act(B, x.H // 2, x.W // 2, x.C, dtype, device)
            a_full = new_act(B, x.H, x.W, x.C, dtype, device) if tab_full is not None else None
            if self.fuse_seams:
                record_hourglass_down(prog, x, pool, a_pool, tab_pool, a_full, tab_full)
            else:
                record_hourglass_down(prog, x, pool)
                if a_full is not None:
                    record_scale_shift_act(prog, x, a_full, *tab_full, "relu")
                record_scale_shift_act(prog, pool, a_pool, *tab_pool, "relu")
            return pool, a_pool, a_full

        def level(i, n, x, tab_next):
            """Level n of hourglass i on the raw map x -> (out, relu(bn_next(out)))."""
            mods, name = self.hg[i].hg[n - 1], f"hg.{i}.hg.{n - 1}"
            pool, a_pool, a_full = down(x, self._bn_table(name + ".1.0.preact.0", mods[1][0].preact[0], dtype, device),
                                        self._bn_table(name + ".0.0.preact.0", mods[0][0].preact[0], dtype, device))
            up1 = chain(name + ".0", mods[0], x, a_full)
            low1 = chain(name + ".1", mods[1], pool, a_pool)
            if n > 1:
                low2, a_low2 = level(i, n - 1, low1, self._bn_table(name + ".2.0.preact.0", mods[2][0].preact[0], dtype, device))
            else:
                low2, a_low2 = chain(name + ".3", mods[3], low1, None), None
            low3 = chain(name + ".2", mods[2], low2, a_low2)
            a_out = new_act(B, up1.H, up1.W, up1.C, dtype, device)
            if self.fuse_seams:
                record_hourglass_up(prog, up1, low3, up1, a_out, tab_next)      # (the sum takes up1's place: nothing else reads up1)
            else:
                record_hourglass_up(prog, up1, low3, up1)
                record_scale_shift_act(prog, up1, a_out, *tab_next, "relu")
            return up1, a_out

        # pre = 7x7/s2/p3 conv + bias + bn + relu on the row-packed input (one kernel row = one K-run), res1, the 2x2 pool, res2, res3
        a_in = new_rowpacked_act(B, H, W, 3, 3, dtype, device)
        record_pack_input(prog, x_static, a_in)
        p = new_act(B, H // 2, W // 2, 64, dtype, device)
        self.fused("pre", self.pre[0].weight, stride=2, pad=3, bias=self.pre[0].bias, bn=self.pre[1].as_dict(), act="relu", **mk).record(prog, a_in, p)
        stages["pre"] = p
        r1 = chain("res1", self.res1, p, p)             # 'no_preact': the block reads the stem's activated map as it is
        stages["res1"] = r1
        pool, a_pool, _ = down(r1, self._bn_table("res2.0.preact.0", self.res2[0].preact[0], dtype, device), None)
        x = chain("res3", self.res3, chain("res2", self.res2, pool, a_pool), None)
        stages["res3"] = x
        K = self.num_classes
        heatmaps = None
        for i in range(self.num_stacks):
            y, a_y = level(i, self.depth, x, self._bn_table(f"res.{i}.0.preact.0", self.res[i][0].preact[0], dtype, device))
            stages[f"hg.{i}"] = y
            y = chain(f"res.{i}", self.res[i], y, a_y)
            y2 = new_act(B, y.H, y.W, self.num_feats, dtype, device)
            self.fused(f"proj.{i}", self.proj[i][0].weight, bias=self.proj[i][0].bias, bn=self.proj[i][1].as_dict(), act="relu", **mk).record(prog, y, y2)
            hm = self.fused(f"heatmap.{i}", self.heatmap[i].weight, bias=self.heatmap[i].bias, act=None, **mk)
            heatmaps = torch.empty((B, K, y.H, y.W), dtype=torch.float32, device=device)
            hm.record(prog, y2, heatmaps)
            stages[f"heatmap.{i}"] = heatmaps
            if i < self.num_stacks - 1:
                # x + proj_(y) + heatmap_(heatmap): the heat map once more as an NHWC map of the compute type (its pad channels
                # [K, 32 k) stay zero: the conv reads them against zero weights), then two convs chained through the residual input
                hm_nhwc = new_act(B, y.H, y.W, K, dtype, device, cstride=(K + 31) // 32 * 32)
                hm.record(prog, y2, hm_nhwc)
                t = new_act(B, y.H, y.W, self.num_feats, dtype, device)
                self.fused(f"proj_.{i}", self.proj_[i].weight, bias=self.proj_[i].bias, act=None, **mk).record(prog, y2, t, residual=x)
                xn = new_act(B, y.H, y.W, self.num_feats, dtype, device)
                self.fused(f"heatmap_.{i}", self.heatmap_[i].weight, bias=self.heatmap_[i].bias, act=None, **mk).record(prog, hm_nhwc, xn, residual=t)
                x = xn
                stages[f"stack.{i}"] = x
        return stages, heatmaps
