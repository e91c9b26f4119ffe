from . import device_pass, flow_utils, net_utils, tracker  # noqa: F401
from .flow_utils import box_propagation, nms  # noqa: F401
from .net_utils import GroupPoseRunner, PoseRunner, detect, flow_est, pose_est, pose_est_frames  # noqa: F401
from .tracker import FlowTracker, HistoryTracker  # noqa: F401
from .device_pass import DeviceTrackingPass  # noqa: F401
from ..detection.test import detect_persons  # noqa: F401
