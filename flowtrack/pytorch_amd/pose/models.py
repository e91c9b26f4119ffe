"""Pose networks of FlowTrack on MI355X: ResNet-50/101/152 trunk + the 3x ConvTranspose(4,2,1) head, the FPN top-down head or the
lateral-deconv head, + 1x1 heatmap conv, executed as fused HIP launches (libflowtrack_hip.so).

Drop-in surface (reference: lib/pose/models/pose_deconv.py:12-63,166-179, pose_fpn.py:48-104,171-184, pose_net.py:30-91,163-177,
resnet.py:15-55, blocks.py:83-120):
    models.deconv(backbone: str, num_classes: int, pretrained: bool) -> module
    models.fpn(backbone: str, num_classes: int, pretrained: bool) -> module
    models.pose(backbone: str, num_classes: int, pretrained: bool) -> module
    models.hg(num_classes: int, num_stacks: int) -> module            (hourglass.py:227-231; forward returns one map per stack)
    module.forward(x[B,3,H,W]) -> heatmaps [B,K,H/4,W/4] (fp32)
    module.state_dict() / load_state_dict() / init_net(path) / .cuda() / .half() / .eval()
with the reference's parameter names and shapes, so its checkpoints
(`ckpt['state_dict']`, tools/pose/main.py:176-181) and torchvision-keyed ImageNet backbones
(`data/pretrained/<backbone>.pth`, loaded strict=False) load unchanged.

What differs by design: eval-mode BatchNorm and ReLU / the residual add are folded into each
conv's epilogue; activations live in NHWC (fp16 or fp32) HBM buffers allocated once per input
shape; the ~60 launches of one forward are replayed as a HIP graph.
"""
from __future__ import annotations

import os

from ..hip_ops import FlowtrackHipError
from ..resnet import BLOCKS
from .densenet import DenseBlock, DenseLayer, FpnDensenet, Transition, densenet_dict          # noqa: F401
from .exact import _ExactHandle                                                                # noqa: F401
from .fpn_head import FpnHead                                                                  # noqa: F401
from .host import PoseHost, PooledStem, _Stages                                                # noqa: F401
from .hourglass import HgBottleneck, Hourglass, HourglassNet                                   # noqa: F401
from .resnet_models import DeconvResnet, FpnResnet, LateralDeconvResnet, PoseResnet            # noqa: F401

resnet_dict = BLOCKS      # depth -> blocks per stage (resnet.py)


def _depth(backbone: str, family: str, table: dict):
    """The NN of `<family>NN` where `table` has it, else None."""
    depth = backbone[len(family):] if backbone.startswith(family) else ""
    return int(depth) if depth.isdigit() and int(depth) in table else None


def _init(model, backbone: str, pretrained: bool):
    """init_net as the reference's factories call it: pretrained=True loads data/pretrained/<backbone>.pth if present."""
    model.init_net(os.path.join("data", "pretrained", "{}.pth".format(backbone)) if pretrained else "")
    return model


def deconv(backbone: str, num_classes: int, pretrained: bool) -> DeconvResnet:
    """Factory with the reference's signature (pose_deconv.py:166-179): backbone 'resnet50' |
    'resnet101' | 'resnet152'; pretrained=True loads data/pretrained/<backbone>.pth if present."""
    if not backbone.startswith("resnet"):
        raise FlowtrackHipError(f"backbone '{backbone}': only the ResNet-50/101/152 + deconv head is on the HIP path")
    depth = int(backbone[len("resnet"):])
    if depth not in resnet_dict:
        raise FlowtrackHipError(f"resnet{depth}: the deconv head needs a Bottleneck trunk (50/101/152)")
    return _init(DeconvResnet(resnet_dict[depth], num_classes=num_classes), backbone, pretrained)


def fpn(backbone: str, num_classes: int, pretrained: bool) -> FpnResnet:
    """Factory with the reference's signature (pose_fpn.py:171-184) for backbone 'resnet50' | 'resnet101' | 'resnet152';
    pretrained=True loads data/pretrained/<backbone>.pth if present.  The reference's DenseNet trunks: fpn_densenet."""
    depth = _depth(backbone, "resnet", resnet_dict)
    if depth is None:
        raise FlowtrackHipError(f"backbone '{backbone}': the FPN head is on the HIP path for resnet50 / resnet101 / resnet152 only" +
                                ("; DenseNet trunks: models.fpn_densenet" if backbone.startswith("densenet") else ""))
    return _init(FpnResnet(resnet_dict[depth], num_classes=num_classes), backbone, pretrained)


#: DenseNet trunks of fpn_densenet.  densenet161 (growth 48) is not among them: its channel windows (144, 240, ...) are no multiples
#: of 32, the K-step of the channel-aligned 3x3 conv kernel that every other trunk's windows run on, and that path has not been
#: validated on such windows
FPN_DENSENETS = ("densenet121", "densenet169", "densenet201")


def fpn_densenet(backbone: str, num_classes: int, pretrained: bool) -> FpnDensenet:
    """The reference's models.fpn on its DenseNet trunks (pose_fpn.py:106-184) for backbone 'densenet121' | 'densenet169' |
    'densenet201'; pretrained=True loads data/pretrained/<backbone>.pth if present (a torchvision checkpoint: its keys are rewritten
    as densenet.py:126-139 rewrites them)."""
    if backbone == "densenet161":
        raise FlowtrackHipError("backbone 'densenet161': growth rate 48 gives channel windows (144, 240, ...) that are no multiples of 32; the 3x3 "
                                f"conv kernel of the HIP path has not been validated on them.  Accepted: {' / '.join(FPN_DENSENETS)}")
    if backbone not in FPN_DENSENETS:
        raise FlowtrackHipError(f"backbone '{backbone}': fpn_densenet takes {' / '.join(FPN_DENSENETS)}")
    return _init(FpnDensenet(*densenet_dict[_depth(backbone, "densenet", densenet_dict)], num_classes=num_classes), backbone, pretrained)


def pose(backbone: str, num_classes: int, pretrained: bool) -> LateralDeconvResnet:
    """Factory with the reference's signature (pose_net.py:163-177) for backbone 'resnet50' | 'resnet101' | 'resnet152';
    pretrained=True loads data/pretrained/<backbone>.pth if present.  The reference's own DenseNet form of this model cannot be
    built (pose_net.py:101 names an undefined `bias`), so there is nothing to follow for it."""
    if backbone.startswith("densenet"):
        raise FlowtrackHipError(f"backbone '{backbone}': the reference itself cannot build this model (PoseDensenet raises NameError: "
                                "name 'bias' is not defined); the lateral-deconv head is on the HIP path for resnet50 / resnet101 / resnet152 only")
    depth = _depth(backbone, "resnet", resnet_dict)
    if depth is None:
        raise FlowtrackHipError(f"backbone '{backbone}': the lateral-deconv head is on the HIP path for resnet50 / resnet101 / resnet152 only")
    return _init(LateralDeconvResnet(resnet_dict[depth], num_classes=num_classes), backbone, pretrained)


def hg(num_classes: int, num_stacks: int) -> HourglassNet:
    """Factory with the reference's signature (hourglass.py:227-231): num_stacks hourglasses of depth 4 on 256 features with
    8 // num_stacks blocks per chain, every conv with bias; the constructor's init is the reference's (there is no checkpoint path)."""
    if isinstance(num_stacks, bool) or not isinstance(num_stacks, int) or not 1 <= num_stacks <= 8:
        raise FlowtrackHipError(f"num_stacks {num_stacks!r}: an integer from 1 to 8 (the reference builds 8 // num_stacks blocks per chain)")
    return HourglassNet(num_classes, num_stacks, 8 // num_stacks)
