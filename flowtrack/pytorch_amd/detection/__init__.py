"""The person detector on the HIP path: the Faster R-CNN networks (nets: resnetv1 and vgg16 on one shared base; test) and their region stage (box NMS, RoI pooling,
crop_and_resize, the proposal layer)."""
from . import nets, ops, proposal, test  # noqa: F401
