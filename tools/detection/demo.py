"""Person detection demo on the HIP path: the Faster R-CNN detector (flowtrack.pytorch_amd.detection.nets: resnetv1 or vgg16) on
one image.

    python tools/detection/demo.py --net res101|vgg16 --model CKPT.pth --num_classes 81 --person_id 1 --image frame.jpg [--fp16]

The image is read with PIL and converted to BGR (the reference reads its frames with cv2.imread); `--model` is a checkpoint of the
reference's detector (a state_dict, or a dict with one under 'state_dict' / 'model'); without it the net runs on the synthetic weights
of flowtrack.pytorch_amd.synth (the boxes are then meaningless, the path is the real one).  Prints the kept person boxes, one
`x1 y1 x2 y2 score` row each, and returns them from main().
"""
from __future__ import absolute_import, division, print_function

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from flowtrack.pytorch_amd import synth   # noqa: E402
from flowtrack.pytorch_amd.detection import nets, test as det_test   # noqa: E402

NETS = {"res50": 50, "res101": 101, "res152": 152, "vgg16": None}        # tools/tracking/demo.py:53-62 of the reference: --detect_net


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--net", default="res101", choices=sorted(NETS), help="trunk")
    parser.add_argument("--model", default="", type=str, metavar="PATH", help="detector checkpoint (default: synthetic weights)")
    parser.add_argument("--num_classes", type=int, default=81, help="classes of the checkpoint, background included")
    parser.add_argument("--person_id", type=int, default=1, help="class id of 'person'")
    parser.add_argument("--image", required=True, type=str, metavar="PATH")
    parser.add_argument("--thresh", type=float, default=0.3, help="NMS threshold of the person boxes")
    parser.add_argument("--target_size", type=int, default=det_test.TEST_SCALE)
    parser.add_argument("--max_size", type=int, default=det_test.TEST_MAX_SIZE)
    parser.add_argument("--fp16", action="store_true", help="run the fp16 mode (default: the fp32 parity mode)")
    parser.add_argument("--seed", type=int, default=1, help="seed of the synthetic weights")
    return parser


def load_image_bgr(path):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def build_net(args):
    net = nets.vgg16() if args.net == "vgg16" else nets.resnetv1(NETS[args.net])
    net.create_architecture(args.num_classes, tag="default")
    fill = synth.fill_vgg_detector_state_dict if args.net == "vgg16" else synth.fill_detector_state_dict
    if args.model:
        ckpt = torch.load(args.model, map_location="cpu")
        for key in ("state_dict", "model"):
            if isinstance(ckpt, dict) and key in ckpt and isinstance(ckpt[key], dict):
                ckpt = ckpt[key]
        net.load_state_dict(ckpt)
    else:
        net.load_state_dict(fill(net.state_dict(), args.seed))
    net = net.cuda().eval()
    net.compute_dtype = torch.float16 if args.fp16 else torch.float32
    return net


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not 0 <= args.person_id < args.num_classes:
        raise SystemExit(f"--person_id {args.person_id} is not a class of a {args.num_classes}-class net")
    net = build_net(args)
    im = load_image_bgr(args.image)
    dets = det_test.detect_persons(net, im, args.person_id, args.thresh, target_size=args.target_size, max_size=args.max_size)
    print(f"{args.image}: {im.shape[0]}x{im.shape[1]}, {len(dets)} person boxes")
    for x1, y1, x2, y2, score in dets:
        print(f"{x1:9.2f} {y1:9.2f} {x2:9.2f} {y2:9.2f} {score:7.4f}")
    return dets


if __name__ == "__main__":
    main()
