"""What the ResNet hosts share (the pose trunks of pose.models, the detector trunk of detection.nets): the Bottleneck parameter
layout, the depth table, and the recorder of one block in every fused form the library has.

The hosts differ in where a block's stride sits and in which forms they offer:
    stride_on="conv2"   the 3x3 carries the stride (blocks.py:83-103, torchvision); inputs are multiples of 32, so a map size is H // s
    stride_on="conv1"   the Caffe layout of the detector (nets/resnet_v1.py:30-35): conv1 carries it, and since a blob has any size a
                        map size is (H - 1) // s + 1 and odd maps occur at every stage
The projection shortcut carries the stride in both.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from .hip_ops import (ActView, FlowtrackHipError, FusedShortcutConv, bottleneck_cluster_supported, bottleneck_entry_fusable, bottleneck_fusable,
                      bottleneck_head_fusable, bottleneck_head_stream_fusable, bottleneck_prefers_fused, bottleneck_strips_supported, new_act,
                      record_bottleneck, record_bottleneck_entry, record_bottleneck_head, record_bottleneck_head_stream)
from .params import ActMarker, BatchNormParams, ConvParams

# depth -> blocks per stage; only Bottleneck nets are valid because the heads hard-code 2048 / 1024
# input channels (pose_deconv.py:20), see SURVEY §8 P1.
BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}

#: every form record_block() knows; a host passes the subset it offers
FORMS = frozenset(("fused",          # an identity block as one launch, recorded as a choice next to its three convs
                   "fused-only",     # ... recorded alone, no choice (dev, tests)
                   "cluster",        # + the four-workgroup cluster form as an option of that choice
                   "strips",         # + the 64-plane register-stationary strip form as an option of that choice
                   "shortcut",       # a projection block's conv3 + shortcut as one K-concatenated GEMM; an unsupported shape raises
                   "shortcut-asked", # ... behind FusedShortcutConv.supported(): plain launches where the library refuses
                   "entry",          # the 64-wide projection block whole, as a choice next to head + GEMM (needs "shortcut")
                   "head",           # conv1 + stride-1 conv2 of the 64-wide projection block as one launch
                   "head2"))         # conv1 + stride-2 conv2 of the 256-plane projection block: a choice of two launches or one


class Bottleneck(nn.Module):
    """Parameter layout of blocks.py:83-103 (stride on the 3x3, torchvision-compatible)."""
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.stride = stride
        self.conv1 = ConvParams(inplanes, planes, 1, bias=False)
        self.bn1 = BatchNormParams(planes)
        self.conv2 = ConvParams(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = BatchNormParams(planes)
        self.conv3 = ConvParams(planes, planes * 4, 1, bias=False)
        self.bn3 = BatchNormParams(planes * 4)
        self.relu = ActMarker("relu")
        if stride != 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(ConvParams(inplanes, planes * 4, 1, stride=stride, bias=False),
                                            BatchNormParams(planes * 4))
        else:
            self.downsample = nn.Sequential()


def conv_out(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def record_block(owner, prog, name: str, blk: Bottleneck, cur: ActView, out: Optional[ActView] = None, *, stride: int, stride_on: str,
                 forms, fallbacks: Optional[list] = None) -> ActView:
    """One Bottleneck (blocks.py:83-120) of `owner` (the HipModule whose layer cache holds the packed weights) from view `cur` into
    view `out` (both may be batch slices of larger buffers; allocated here when None), in the forms of `forms` (a subset of FORMS)
    the library takes for the shape: where two forms exist both are recorded as a choice and the first-call benchmark keeps one.
    `fallbacks`, when given, collects the names of the blocks that an offered form would cover and the library refused at this
    shape (fp16 identity blocks on plain launches, projection blocks whose shortcut query said no).  Returns `out`."""
    if stride_on not in ("conv1", "conv2") or not FORMS.issuperset(forms):
        raise FlowtrackHipError(f"{name}: stride_on {stride_on!r} / forms {sorted(set(forms) - FORMS)} unknown")
    dtype, device = cur.t.dtype, cur.t.device
    N, mk = cur.N, dict(dtype=dtype, device=device)
    planes, s, on1 = blk.conv1.cout, stride, stride_on == "conv1"
    Ho, Wo = (conv_out(cur.H, 1, s, 0), conv_out(cur.W, 1, s, 0)) if on1 else (cur.H // s, cur.W // s)
    H1, W1 = (Ho, Wo) if on1 else (cur.H, cur.W)        # conv1's output
    c1 = owner.fused(name + ".conv1", blk.conv1.weight, stride=s if on1 else 1, bn=blk.bn1.as_dict(), act="relu", **mk)
    c2 = owner.fused(name + ".conv2", blk.conv2.weight, stride=1 if on1 else s, pad=1, bn=blk.bn2.as_dict(), act="relu", **mk)
    c3 = owner.fused(name + ".conv3", blk.conv3.weight, bn=blk.bn3.as_dict(), act="relu", **mk)
    if out is None:
        out = new_act(N, Ho, Wo, planes * 4, dtype, device)
    projection = bool(len(blk.downsample))
    if not projection and s == 1 and ("fused" in forms or "fused-only" in forms):
        if bottleneck_fusable(c1, c2, c3, cur, out):
            if "fused-only" in forms:
                record_bottleneck(prog, c1, c2, c3, cur, out, name + ".fused", form="patch")
                return out
            # the whole block in one launch (t1 / t2 never leave LDS) or as three conv launches: which one is faster
            # depends on how many workgroups the stage's pixels make (each streams the block's whole weight set),
            # so both are recorded and the first-call benchmark keeps one (Program.tune_choices)
            t1 = new_act(N, H1, W1, planes, dtype, device)
            t2 = new_act(N, Ho, Wo, planes, dtype, device)

            def conv_form():
                c1.record(prog, cur, t1)
                c2.record(prog, t1, t2)
                c3.record(prog, t2, out, residual=cur)
            options = (("fused", lambda: record_bottleneck(prog, c1, c2, c3, cur, out, name + ".fused", form="patch")), ("convs", conv_form))
            if not bottleneck_prefers_fused(cur, planes):
                options = options[::-1]
            if "cluster" in forms and bottleneck_cluster_supported(cur, out, planes):
                # round 5: the same block shared by a cluster of four workgroups per image (t1 / t2 exchanged inside the
                # launch): a third recorded form, kept where the first-call benchmark measures it faster
                options = options + (("cluster", lambda: record_bottleneck(prog, c1, c2, c3, cur, out, name + ".cluster", cluster=True)),)
            if "strips" in forms and planes == 64 and bottleneck_strips_supported(cur, out, planes):
                # round 5: the 64-plane block on register-stationary strips (csrc/bottleneck_rstat.hip): 54 against 57.5 us alone
                # and with warm caches, 59-63 against ~55 us behind a cold L2 (its prologue waits for 139 KB of weights before the
                # first x load): recorded only with FT_STRIP_KERNELS=1 — the first-call benchmark times a group's later options
                # behind warmer caches than its first, a bias larger than this form's margin
                strips = (("strips", lambda: record_bottleneck(prog, c1, c2, c3, cur, out, name + ".strips", form="strips")),)
                options = strips + options if os.environ.get("FT_STRIP_KERNELS") == "2" else options + strips      # (2: the first choice, dev)
            prog.begin_choice(f"bottleneck|{N},{cur.H},{cur.W},{cur.C},{planes},{cur.cstride},{out.cstride}")
            for option_name, option in options:
                prog.option(option_name)
                option()
            prog.end_choice()
            return out
        if fallbacks is not None and dtype == torch.float16:
            fallbacks.append(name)
    t2 = new_act(N, Ho, Wo, planes, dtype, device)
    sc = None
    if projection and "shortcut" in forms:
        sc = owner.fused_shortcut(name + ".conv3+downsample", blk, s, **mk)
    elif projection and "shortcut-asked" in forms:
        if FusedShortcutConv.supported(blk.conv3.cin, blk.downsample[0].cin, blk.conv3.cout, s, dtype, t2, cur, out):
            sc = owner.fused_shortcut(name + ".conv3+downsample", blk, s, **mk)
        elif fallbacks is not None:
            fallbacks.append(name)
    whole = "entry" in forms and sc is not None and bottleneck_entry_fusable(c1, c2, sc, cur, out)
    if whole:
        # the 64-wide entry block whole (t1, t2 and the shortcut never leave the CU) or as head + K-concatenated
        # conv3: both recorded, the first-call benchmark keeps one
        prog.begin_choice(f"entry|{N},{cur.H},{cur.W},{cur.C},{planes},{cur.cstride},{out.cstride}")
        prog.option("fused")
        record_bottleneck_entry(prog, c1, c2, sc, cur, out, name + ".fused")
        prog.option("head+exit")
    if "head" in forms and s == 1 and bottleneck_head_fusable(c1, c2, cur, t2):
        record_bottleneck_head(prog, c1, c2, cur, t2, name + ".conv1+conv2")   # the 64-wide entry block: t1 in LDS only
    else:
        head2 = "head2" in forms and s == 2 and bottleneck_head_stream_fusable(c1, c2, cur, t2)
        if head2:
            # the 256-plane entry block's conv1 + stride-2 conv2 as one streamed-weights launch, or as two launches:
            # both recorded, the first-call benchmark keeps one (the recorder's first choice: two launches)
            prog.begin_choice(f"head2|{N},{cur.H},{cur.W},{cur.C},{planes},{cur.cstride},{t2.cstride}")
            prog.option("convs")
        t1 = new_act(N, H1, W1, planes, dtype, device)
        c1.record(prog, cur, t1)
        c2.record(prog, t1, t2)
        if head2:
            prog.option("fused")
            record_bottleneck_head_stream(prog, c1, c2, cur, t2, name + ".conv1+conv2")
            prog.end_choice()
    if sc is not None:
        # conv3 + bn3 and the projection shortcut as one GEMM over K = [t2 | block input] (blocks.py:104-119):
        # the shortcut tensor never exists in HBM
        sc.record(prog, t2, cur, out)
    elif projection:
        ds = owner.fused(name + ".downsample", blk.downsample[0].weight, stride=s, bn=blk.downsample[1].as_dict(), act=None, **mk)
        res = new_act(N, Ho, Wo, planes * 4, dtype, device)
        ds.record(prog, cur, res)
        c3.record(prog, t2, out, residual=res)
    else:
        c3.record(prog, t2, out, residual=cur)  # relu(bn3(conv3) + residual), blocks.py:114-119
    if whole:
        prog.end_choice()
    return out
