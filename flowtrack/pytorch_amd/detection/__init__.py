"""The person detector on the HIP path: the Faster R-CNN network (nets, test) and its region stage (box NMS, RoI pooling,
crop_and_resize, the proposal layer)."""
from . import nets, ops, proposal, test  # noqa: F401
