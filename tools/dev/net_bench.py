"""Per-launch timing of a whole plan (dev tool): python tools/dev/net_bench.py FlowNet2C 16 384 512 fp16
(pose nets: resnet50 = ResNet-50 + deconv head, fpn_resnet50 = ResNet-50 + FPN head, pose_resnet50 = ResNet-50 + lateral-deconv head,
fpn_densenet121 = DenseNet-121 + FPN head, hg8 = 8 stacked hourglasses; NB_FUSE_SEAMS=0 records the hourglass's level seams unfused)"""
import sys, os, types
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from flowtrack.pytorch_amd import synth


def frcnn(name, H, W, dt):
    """python tools/dev/net_bench.py frcnn_resnet101|frcnn_vgg16 600 1000 [fp16]: the detector on one H x W blob (a uint8 frame of that size at
    scale 1): the per-launch tables of the trunk + RPN plan and of the region-head plan, then the per-image time of the three steps."""
    import time
    import numpy as np
    from flowtrack.pytorch_amd.detection import nets, test as det_test
    vgg = name == "frcnn_vgg16"
    net = nets.vgg16() if vgg else nets.resnetv1(int(name[len("frcnn_resnet"):]))
    net.create_architecture(81, tag="default")
    net.load_state_dict((synth.fill_vgg_detector_state_dict if vgg else synth.fill_detector_state_dict)(net.state_dict(), 1))
    net = net.cuda().eval()
    net.compute_dtype = torch.float16 if dt == "fp16" else torch.float32
    frame = torch.from_numpy(synth.detector_frame(1, H, W)).cuda()
    kw = dict(target_size=min(H, W), max_size=max(H, W))
    for _ in range(3):
        dets = det_test.detect_persons(net, frame, 1, 0.3, **kw)
    torch.cuda.synchronize()
    plan, im_info, _, shape = det_test.stage_frame(net, frame, **kw)
    head = next(iter(plan.heads.values()))
    print(f"{name} {dt}: blob {tuple(plan.x_static.shape[2:])}, net_conv {plan.net_conv.H}x{plan.net_conv.W}, {int(net._predictions['rois'].shape[0])} RoIs, "
          f"{len(dets)} person boxes; blocks on plain launches: trunk {plan.fallbacks or 'none'}, head {head.fallbacks or 'none'}")
    glue = {"ft_rpn_softmax_fwd", "ft_rcnn_mean_pool_fwd", "ft_maxpool2x2s2_fwd", "ft_fc_fwd"}
    for what, prog in (("trunk + RPN", plan.prog), ("region head", head.prog)):
        labels = {idx: lab for lab, idx, _, _ in prog.conv_records}
        labels.update({r[1]: r[0] for r in prog.fused_records})
        tot = new = 0.0
        print(f"-- {what} plan")
        for i, (nm, ms) in enumerate(prog.time_calls(iters=5)):
            if nm.startswith("__"): continue
            tot += ms
            new += ms if nm in glue else 0.0
            print(f"{i:3d} {nm:28s} {labels.get(i, ''):36s} {ms*1e3:9.1f} us")
        print(f"sum of launches {tot:.3f} ms, of which the new glue kernels {new*1e3:.1f} us")

    def timed(fn, n=20):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n): out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, out
    from flowtrack.pytorch_amd.detection import proposal
    t_blob, _ = timed(lambda: det_test.stage_frame(net, frame, **kw))
    t_trunk, _ = timed(lambda: net.run(plan))
    t_prop, (rois, _) = timed(lambda: proposal.proposal_layer(plan.rpn_cls_prob, plan.rpn_bbox_pred, im_info, "TEST", 16, plan.anchors, net._num_anchors))
    t_head, _ = timed(lambda: net.region_head(plan, rois, float(im_info[2]), shape))
    t_hplan, _ = timed(lambda: net.run(head))
    t_all, _ = timed(lambda: det_test.detect_persons(net, frame, 1, 0.3, **kw))
    print(f"per image: ft_detect_blob_fwd {t_blob:.3f} ms, trunk + RPN plan (graph) {t_trunk:.3f} ms, proposal step {t_prop:.3f} ms, region head {t_head:.3f} ms "
          f"(its plan alone {t_hplan:.3f} ms; the rest: RoI staging + ft_rcnn_detections_fwd), detect_persons end to end {t_all:.3f} ms")


if sys.argv[1].startswith("frcnn_"):
    frcnn(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] if len(sys.argv) > 4 else "fp16")
    sys.exit(0)
name, B, H, W, dt = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
dtype = torch.float16 if dt == "fp16" else torch.float32
if name.startswith("hg"):        # hg8 = models.hg(17, num_stacks=8)
    from flowtrack.pytorch_amd.pose import models
    m = models.hg(17, int(name[2:]))
    m.fuse_seams = os.environ.get("NB_FUSE_SEAMS", "1") != "0"
    m.load_state_dict(synth.fill_hg_state_dict(m.state_dict(), 1))
    x = synth.pose_crops(1, B, H, W)
elif name.startswith("fpn_densenet"):          # fpn_densenet121: the FPN head on a DenseNet trunk; NB_DENSE_LAYER pins a dense-layer form
    from flowtrack.pytorch_amd.pose import models
    m = models.fpn_densenet(name[4:], 17, False)
    m.dense_layer_form = os.environ.get("NB_DENSE_LAYER") or m.dense_layer_form
    m.load_state_dict(synth.fill_densenet_state_dict(m.state_dict(), 1))
    x = synth.pose_crops(1, B, H, W)
elif name.startswith(("resnet", "fpn_resnet", "pose_resnet")):      # resnet50 = the deconv head, fpn_resnet50 = the FPN head, pose_resnet50 = the lateral-deconv head
    from flowtrack.pytorch_amd.pose import models
    m = models.fpn(name[4:], 17, False) if name.startswith("fpn_") else models.pose(name[5:], 17, False) if name.startswith("pose_") else models.deconv(name, 17, False)
    m.load_state_dict(synth.fill_pose_state_dict(m.state_dict(), 1))
    x = synth.pose_crops(1, B, H, W)
else:
    from flowtrack.pytorch_amd.flownet import models
    m = getattr(models, name)(types.SimpleNamespace(rgb_max=255.0, fp16=False)); m.load_state_dict(synth.fill_flow_state_dict(m.state_dict(), 1))
    x = synth.frame_pairs(1, B, H, W)
m = m.cuda().eval(); m.compute_dtype = dtype
x = x.cuda()
for _ in range(3): m(x)
torch.cuda.synchronize()
plan = next(iter(m._plans.values()))
times = plan.prog.time_calls(iters=5)
hot = dict(enumerate(t for _, t in plan.prog.time_calls(iters=5, repeat_hot=True))) if os.environ.get("NB_HOT") else {}
labels = {idx: lab for lab, idx, _, _ in plan.prog.conv_records}
labels.update({r[1]: r[0] for r in plan.prog.fused_records})
flops = {r[1]: r[2] for r in list(plan.prog.conv_records) + list(plan.prog.fused_records)}
tot = 0.0
for i, (nm, ms) in enumerate(times):
    tot += ms
    if nm.startswith("__"): continue
    print(f"{i:3d} {nm:28s} {labels.get(i, ''):28s} {ms*1e3:9.1f} us" + (f"  {flops[i] / ms * 1e-9:7.1f} TF/s" if i in flops else "")
          + (f"   hot {hot[i]*1e3:7.1f} us  (cold - hot {1e3 * (ms - hot[i]):+6.1f})" if hot else ""))
print(f"sum of launches {tot:.3f} ms  -> {B/tot*1e3:.0f} units/s (eager, event-timed)")
import time
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20): m(x, copy_output=False)
torch.cuda.synchronize(); dt_ = (time.perf_counter() - t0) / 20
print(f"graph replay {dt_*1e3:.3f} ms/step -> {B/dt_:.0f} units/s")
