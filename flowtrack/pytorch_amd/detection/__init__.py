"""The person detector's region stage on the HIP path: box NMS, RoI pooling, crop_and_resize, the proposal layer."""
from . import ops, proposal  # noqa: F401
