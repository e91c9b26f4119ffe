"""The launch list of a plan as text (dev tool): builds the plan without running it and prints one line per entry of prog.calls —
call name, lane, every argument — then conv_records, fused_records and, for the detector, the blocks on plain launches.  Two trees
record the same plan exactly when their dumps are byte-equal: a device address (any integer >= 2**32) is printed as the ordinal of
its first appearance in the dump, so the text does not depend on the allocator and still pins which launch reads which buffer.

    python tools/dev/plan_dump.py SPEC [SPEC ...]         SPEC = name:B:H:W:dtype[:variant]
    resnet50:64:256:192:fp16          models.deconv (fpn_resnet50 / pose_resnet50: the FPN / lateral-deconv head; fpn_densenet121; hg2: 2 hourglasses)
    resnet50:64:256:192:fp16:flip     the flip plan of the shape
    resnet50:64:256:192:fp16:kp       a pose model's plan with keypoints_in_plan = True (its last launch writes the key-point rows)
    resnet50:64:256:192:fp16:exact    ... and exact_in_plan = True (fp16: the exact-arg-max screen, gather and header copy behind it)
    frcnn_resnet50:1:600:901:fp16     the detector's trunk + RPN plan of one H x W blob and its region-head plan at 300 rows
    frcnn_resnet50:1:600:901:fp16:force    ... with fuse_bottleneck = "force"
    FlowNet2S:2:128:128:fp32          a flow model
The recorder's switches (FT_SPLIT_LANES, FT_FUSE_STAGE_EXIT, ...) are read from the environment when the package is imported."""
import ctypes, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from flowtrack.pytorch_amd import synth

FLIP_PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]


class Dumper:
    def __init__(self):
        self.addresses = {}

    def arg(self, a):
        if hasattr(a, "_obj"):                      # ctypes.byref(struct)
            a = a._obj
        if isinstance(a, ctypes.Structure):         # ConvDesc, BottleneckDesc: geometry only
            return bytes(a).hex()
        if isinstance(a, ctypes._SimpleCData):
            a = a.value
        if isinstance(a, int) and not isinstance(a, bool) and a >= 2 ** 32:
            return f"@{self.addresses.setdefault(a, len(self.addresses))}"
        return repr(a) if isinstance(a, float) else str(a)

    def prog(self, title, prog, fallbacks=None):
        print(f"-- {title}: {len(prog.calls)} calls")
        for i, ((name, args), lane) in enumerate(zip(prog.calls, prog.lanes)):
            print(f"{i:4d} {name} lane={lane} " + " ".join(self.arg(a) for a in args))
        for label, idx, flops, d in prog.conv_records:
            print(f"conv_record {label} {idx} {flops!r} {bytes(d).hex()}")
        for rec in prog.fused_records:
            print("fused_record " + " ".join(self.arg(v) for v in rec))
        if fallbacks is not None:
            print(f"fallbacks {fallbacks}")


def dump(spec):
    name, B, H, W, dt, *variant = spec.split(":")
    B, H, W, variant = int(B), int(H), int(W), variant[0] if variant else ""
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dt]
    print(f"## {spec}")
    out = Dumper()
    if name.startswith("frcnn_resnet"):
        from flowtrack.pytorch_amd.detection import nets
        net = nets.resnetv1(int(name[len("frcnn_resnet"):]))
        net.create_architecture(81, tag="default")
        net.load_state_dict(synth.fill_detector_state_dict(net.state_dict(), 1))
        net = net.cuda().eval()
        net.compute_dtype = dtype
        if variant == "force":
            net.fuse_bottleneck = "force"
        trunk = net.trunk_plan(H, W)
        head = net.head_plan(trunk, 300)
        out.prog(f"trunk + RPN, net_conv {trunk.net_conv.H}x{trunk.net_conv.W}", trunk.prog, trunk.fallbacks)
        out.prog("region head", head.prog, head.fallbacks)
        return
    if name.startswith("hg"):
        from flowtrack.pytorch_amd.pose import models
        m = models.hg(17, int(name[2:]))
        m.load_state_dict(synth.fill_hg_state_dict(m.state_dict(), 1))
    elif name.startswith("fpn_densenet"):          # fpn_densenet121: the FPN head on a DenseNet trunk; NB_DENSE_LAYER pins a dense-layer form
        from flowtrack.pytorch_amd.pose import models
        m = models.fpn_densenet(name[4:], 17, False)
        m.dense_layer_form = os.environ.get("NB_DENSE_LAYER") or m.dense_layer_form
        m.load_state_dict(synth.fill_densenet_state_dict(m.state_dict(), 1))
    elif name.startswith(("resnet", "fpn_resnet", "pose_resnet")):
        from flowtrack.pytorch_amd.pose import models
        m = models.fpn(name[4:], 17, False) if name.startswith("fpn_") else models.pose(name[5:], 17, False) if name.startswith("pose_") else models.deconv(name, 17, False)
        m.load_state_dict(synth.fill_pose_state_dict(m.state_dict(), 1))
        if variant == "flip":
            m.flip_pairs = FLIP_PAIRS
    else:
        from flowtrack.pytorch_amd.flownet import models
        m = getattr(models, name)(types.SimpleNamespace(rgb_max=255.0, fp16=False))
        m.load_state_dict(synth.fill_flow_state_dict(m.state_dict(), 1))
    if variant in ("kp", "exact"):                  # (pose models) the plan's tail as well: key points, and the exact-arg-max screen
        m.keypoints_in_plan, m.exact_in_plan = True, variant == "exact"
    m = m.cuda().eval()
    m.compute_dtype = dtype
    m.static_input(B, H, W)                        # builds the plan, runs nothing
    (key, plan), = m._plans.items()
    out.prog(f"plan {[k for k in key if not isinstance(k, torch.device)]}", plan.prog)


for spec in sys.argv[1:]:
    dump(spec)
    torch.cuda.empty_cache()
