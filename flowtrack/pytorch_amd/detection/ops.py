"""Drop-ins for the detector's three native operator packages (reference lib/detection).

The reference binds box NMS (nms/pth_nms.py), RoI pooling (layer_utils/roi_pooling/roi_pool.py) and crop_and_resize
(layer_utils/roi_align/crop_and_resize.py) as cffi `_ext` modules.  These keep the reference's signatures, so its call sites
(nets/network.py:91,117, model/nms_wrapper.py) work unchanged; forward runs ft_*_fwd and backward ft_*_bwd
(include/flowtrack_hip.h) on the current stream.  Inputs must be fp32 CUDA tensors; there is no CPU or half-precision path.
Both backward passes sum with float atomics: the crop_and_resize image gradient can differ in the last bits from run to run,
the RoI-pool gradient only where several RoIs pooled the same element.

    from flowtrack.pytorch_amd.detection.ops import nms, RoIPoolFunction, CropAndResizeFunction
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import FlowtrackHipError, check

__all__ = ["nms", "box_nms_sorted", "RoIPoolFunction", "RoIPool", "CropAndResizeFunction", "CropAndResize"]

NMS_MAX_BOXES = 16384


def _fp32_cuda(t, name: str, shape) -> torch.Tensor:
    """`shape`: one entry per dimension, None where any size is accepted."""
    if not isinstance(t, torch.Tensor):
        raise FlowtrackHipError(f"{name}: the HIP operators take fp32 CUDA tensors, got {type(t).__name__}")
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        want = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
        raise FlowtrackHipError(f"{name}: expected a tensor of shape {want}, got {tuple(t.shape)}")
    if not t.is_cuda or t.dtype != torch.float32:
        raise FlowtrackHipError(f"{name}: the HIP operators take fp32 CUDA tensors, got {t.dtype} on {t.device}")
    return t.contiguous()


def _stream(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def box_nms_sorted(dets: torch.Tensor, thresh: float, inclusive: bool = False, max_keep: int = 0):
    """ft_box_nms on score-descending `dets` [n,5]: (keep int32[n] with -1 past the count, count int32[1]), both on the
    device; nothing is read back."""
    dets = _fp32_cuda(dets, "box_nms_sorted dets", (None, 5))
    n = dets.shape[0]
    keep = torch.empty(n, dtype=torch.int32, device=dets.device)
    count = torch.zeros(1, dtype=torch.int32, device=dets.device)
    if n == 0:
        return keep, count
    lib = _lib.load()
    if n > NMS_MAX_BOXES:
        raise FlowtrackHipError(f"box NMS: {n} boxes, the kernel takes at most {NMS_MAX_BOXES}")
    workspace = torch.empty(lib.ft_box_nms_workspace_bytes(n), dtype=torch.uint8, device=dets.device)
    with torch.cuda.device(dets.device):
        check(lib.ft_box_nms(_ptr(dets), n, float(thresh), int(bool(inclusive)), int(max_keep), _ptr(workspace), _ptr(keep), _ptr(count),
                             _stream(dets.device)), "ft_box_nms")
    return keep, count


def nms(dets: torch.Tensor, thresh: float) -> torch.Tensor:
    """nms/pth_nms.py for a CUDA tensor: sorts by score, suppresses on IoU > thresh, returns a LongTensor of indices into `dets`
    in kept order."""
    dets = _fp32_cuda(dets, "nms dets", (None, 5))
    if dets.shape[0] == 0:
        return torch.empty(0, dtype=torch.long, device=dets.device)
    order = dets[:, 4].sort(dim=0, descending=True, stable=True)[1]
    keep, count = box_nms_sorted(dets[order], thresh)
    return order[keep[:int(count.item())].long()].contiguous()


class _RoIPool(Function):
    @staticmethod
    def forward(ctx, features, rois, pooled_height, pooled_width, spatial_scale):
        features = _fp32_cuda(features, "RoIPool features", (None,) * 4)
        rois = _fp32_cuda(rois, "RoIPool rois", (None, 5))
        if rois.device != features.device:
            raise FlowtrackHipError(f"RoIPool: features on {features.device}, rois on {rois.device}")
        B, C, H, W = features.shape
        R = rois.shape[0]
        out = torch.empty((R, C, pooled_height, pooled_width), dtype=torch.float32, device=features.device)
        argmax = torch.empty((R, C, pooled_height, pooled_width), dtype=torch.int32, device=features.device)
        with torch.cuda.device(features.device):
            check(_lib.load().ft_roi_pool_fwd(_ptr(features), _ptr(rois), B, C, H, W, R, spatial_scale, pooled_height, pooled_width,
                                              _ptr(out), _ptr(argmax), _stream(features.device)), "ft_roi_pool_fwd")
        ctx.save_for_backward(rois, argmax)
        ctx.feature_size = (B, C, H, W)
        ctx.pooled = (pooled_height, pooled_width)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        rois, argmax = ctx.saved_tensors
        B, C, H, W = ctx.feature_size
        R = rois.shape[0]
        grad_output = _fp32_cuda(grad_output, "RoIPool grad_output", (R, C) + ctx.pooled)
        grad_input = torch.empty(ctx.feature_size, dtype=torch.float32, device=grad_output.device)
        with torch.cuda.device(grad_output.device):
            check(_lib.load().ft_roi_pool_bwd(_ptr(grad_output), _ptr(rois), _ptr(argmax), B, C, H, W, R, *ctx.pooled, _ptr(grad_input),
                                              _stream(grad_output.device)), "ft_roi_pool_bwd")
        return grad_input, None, None, None, None


class RoIPoolFunction:
    """roi_pooling/roi_pool.py: `RoIPoolFunction(ph, pw, scale)(features, rois)`."""

    def __init__(self, pooled_height, pooled_width, spatial_scale):
        self.pooled_width = int(pooled_width)
        self.pooled_height = int(pooled_height)
        self.spatial_scale = float(spatial_scale)

    def __call__(self, features, rois):
        return _RoIPool.apply(features, rois, self.pooled_height, self.pooled_width, self.spatial_scale)


class RoIPool(nn.Module):
    """roi_pooling/roi_pool.py: the module form."""

    def __init__(self, pooled_height, pooled_width, spatial_scale):
        super().__init__()
        self.pooled_width = int(pooled_width)
        self.pooled_height = int(pooled_height)
        self.spatial_scale = float(spatial_scale)

    def forward(self, features, rois):
        return RoIPoolFunction(self.pooled_height, self.pooled_width, self.spatial_scale)(features, rois)


class _CropAndResize(Function):
    @staticmethod
    def forward(ctx, image, boxes, box_ind, crop_height, crop_width, extrapolation_value):
        image = _fp32_cuda(image, "CropAndResize image", (None,) * 4)
        boxes = _fp32_cuda(boxes, "CropAndResize boxes", (None, 4))
        R = boxes.shape[0]
        if not isinstance(box_ind, torch.Tensor) or not box_ind.is_cuda or box_ind.dtype != torch.int32 or tuple(box_ind.shape) != (R,):
            what = f"{box_ind.dtype} {tuple(box_ind.shape)} on {box_ind.device}" if isinstance(box_ind, torch.Tensor) else type(box_ind).__name__
            raise FlowtrackHipError(f"CropAndResize box_ind: expected an int32 CUDA tensor of shape [{R}], got {what}")
        if boxes.device != image.device or box_ind.device != image.device:
            raise FlowtrackHipError(f"CropAndResize: image on {image.device}, boxes on {boxes.device}, box_ind on {box_ind.device}")
        box_ind = box_ind.contiguous()
        B, C, H, W = image.shape
        crops = torch.empty((R, C, crop_height, crop_width), dtype=torch.float32, device=image.device)
        with torch.cuda.device(image.device):
            check(_lib.load().ft_crop_and_resize_fwd(_ptr(image), _ptr(boxes), _ptr(box_ind), B, C, H, W, R, crop_height, crop_width,
                                                     extrapolation_value, _ptr(crops), _stream(image.device)), "ft_crop_and_resize_fwd")
        ctx.save_for_backward(boxes, box_ind)
        ctx.im_size = (B, C, H, W)
        ctx.crop = (crop_height, crop_width)
        return crops

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_outputs):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        boxes, box_ind = ctx.saved_tensors
        B, C, H, W = ctx.im_size
        R = boxes.shape[0]
        grad_outputs = _fp32_cuda(grad_outputs, "CropAndResize grad_outputs", (R, C) + ctx.crop)
        grad_image = torch.empty(ctx.im_size, dtype=torch.float32, device=grad_outputs.device)
        with torch.cuda.device(grad_outputs.device):
            check(_lib.load().ft_crop_and_resize_bwd(_ptr(grad_outputs), _ptr(boxes), _ptr(box_ind), B, C, H, W, R, *ctx.crop,
                                                     _ptr(grad_image), _stream(grad_outputs.device)), "ft_crop_and_resize_bwd")
        return grad_image, None, None, None, None, None


class CropAndResizeFunction:
    """roi_align/crop_and_resize.py: `CropAndResizeFunction(ch, cw, extrapolation_value=0)(image, boxes, box_ind)`."""

    def __init__(self, crop_height, crop_width, extrapolation_value=0):
        self.crop_height = int(crop_height)
        self.crop_width = int(crop_width)
        self.extrapolation_value = float(extrapolation_value)

    def __call__(self, image, boxes, box_ind):
        return _CropAndResize.apply(image, boxes, box_ind, self.crop_height, self.crop_width, self.extrapolation_value)


class CropAndResize(nn.Module):
    """roi_align/crop_and_resize.py: the module form."""

    def __init__(self, crop_height, crop_width, extrapolation_value=0):
        super().__init__()
        self.crop_height = crop_height
        self.crop_width = crop_width
        self.extrapolation_value = extrapolation_value

    def forward(self, image, boxes, box_ind):
        return CropAndResizeFunction(self.crop_height, self.crop_width, self.extrapolation_value)(image, boxes, box_ind)
