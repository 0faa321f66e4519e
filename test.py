#!/usr/bin/env python
"""test.py -- evaluation entry point mirroring the reference's test.py (test() :17-201, flags :205-217):
forward (HIP engine) -> non_max_suppression -> greedy matching on rotated IoU -> ap_per_class.
The reference matches predictions with a per-pair Python + shapely loop (test.py:134-151, utils/utils.py:290-320);
here one `ryolo_eval_match` call per batch (three launches, one device -> host transfer), or with batched_match=False one
`ryolo_skew_iou_matrix` launch and a host loop per image.  Data: the synthetic loader, or with --real-data the `valid` image list of
--data through the device loader (utils/datasets.py, csrc/augment.hip: letterbox only, no augmentation)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd.model.models import Darknet  # noqa: E402
from rotate_yolov3_amd.utils.metrics import ap_per_class, match_predictions, match_predictions_batched  # noqa: E402
from rotate_yolov3_amd.utils.nms.nms import check_nms_style  # noqa: E402
from rotate_yolov3_amd.utils.nms.nms import non_max_suppression_batched as non_max_suppression  # noqa: E402  (same rows, one segmented NMS launch per batch; CPU tensors take the loop)
from rotate_yolov3_amd.utils.parse_config import hyp_parse  # noqa: E402
from rotate_yolov3_amd.utils.synthetic import SyntheticLoader  # noqa: E402


def _batch_stats(stats, inf_out, targets, width, height, iou_thres, conf_thres, nms_thres, nms_style='OR'):
    """The statistics of one batch, appended to `stats` in the order of the per-image loop of test(): one NMS call, one matcher call, ONE
    device -> host transfer (flags, scores and classes of all predictions, and below them the image and class of every target)."""
    bs = len(inf_out)
    output, det, det_off = non_max_suppression(inf_out, conf_thres=conf_thres, nms_thres=nms_thres, flat=True, nms_style=nms_style)
    labels = targets.clone()
    labels[:, [2, 4]] *= width
    labels[:, [3, 5]] *= height
    correct, _ = match_predictions_batched(det, det_off, labels, bs, iou_thres)
    host = torch.cat((torch.stack((correct.float(), det[:, 5], det[:, 7]), 1),
                      torch.nn.functional.pad(targets[:, :2], (0, 1))), 0).cpu()
    rows, tgt = host[:len(det)], host[len(det):]
    start = 0
    for si, pred in enumerate(output):
        tcls = tgt[tgt[:, 0] == si, 1].tolist()
        if pred is None:
            if tcls:
                stats.append(([], torch.Tensor(), torch.Tensor(), tcls))
            continue
        r = rows[start:start + len(pred)]
        start += len(pred)
        stats.append((r[:, 0].long().tolist(), r[:, 1], r[:, 2], tcls))
    return bs


def test(cfg, hyp, weights=None, batch_size=16, img_size=608, iou_thres=0.5, conf_thres=0.001, nms_thres=0.5, model=None,
         n_images=32, device=None, nc=None, batched_match=True, loader=None, nms_style='OR'):
    """loader: batches to evaluate (utils.datasets.LoadImagesAndLabels); None: n_images synthetic ones;
    nms_style: 'OR' or 'MERGE' (utils/nms/nms.py)"""
    check_nms_style(nms_style)
    device = device or torch.device('cuda:0')
    if model is None:
        model = Darknet(cfg, hyp)
        if weights and weights.endswith('.pt'):
            model.load_state_dict(torch.load(weights, map_location='cpu')['model'])
        elif weights:                                # darknet format (reference test.py:47-48)
            from rotate_yolov3_amd.model.model_utils import load_darknet_weights
            load_darknet_weights(model, weights)
        model.to(device)
    model.eval()
    nc = int(nc) if nc else model.nc
    seen = 0
    stats = []
    with torch.no_grad():
        for imgs, targets, _, _ in (loader if loader is not None else SyntheticLoader(n_images, batch_size, img_size, seed=1, device=device)):
            _, _, height, width = imgs.shape
            inf_out, train_out = model(imgs)
            if batched_match:
                seen += _batch_stats(stats, inf_out, targets, width, height, iou_thres, conf_thres, nms_thres, nms_style)
                continue
            output = non_max_suppression(inf_out, conf_thres=conf_thres, nms_thres=nms_thres, nms_style=nms_style)
            for si, pred in enumerate(output):
                labels = targets[targets[:, 0] == si, 1:].clone()
                nl = len(labels)
                tcls = labels[:, 0].tolist() if nl else []
                seen += 1
                if pred is None:
                    if nl:
                        stats.append(([], torch.Tensor(), torch.Tensor(), tcls))
                    continue
                if nl:
                    labels[:, [1, 3]] *= width
                    labels[:, [2, 4]] *= height
                correct = match_predictions(pred, labels, iou_thres)
                stats.append((correct, pred[:, 5].cpu(), pred[:, 7].cpu(), tcls))
    stats = [np.concatenate(x, 0) for x in list(zip(*stats))] if stats else []
    if len(stats):
        p, r, ap, f1, ap_class = ap_per_class(*stats)
        mp, mr, map_, mf1 = p.mean(), r.mean(), ap.mean(), f1.mean()
        nt = np.bincount(stats[3].astype(np.int64), minlength=nc)
    else:
        mp = mr = map_ = mf1 = 0.
        nt = np.zeros(1)
        ap, ap_class = [], []
    print(('%20s' + '%10s' * 6) % ('Class', 'Images', 'Targets', 'P', 'R', 'mAP', 'F1'))
    print(('%20s' + '%10.3g' * 6) % ('all', seen, nt.sum(), mp, mr, map_, mf1))
    maps = np.zeros(nc) + map_
    for i, c in enumerate(ap_class):
        maps[c] = ap[i]
    return (mp, mr, map_, mf1, 0., 0., 0.), maps


def build_parser():
    """-> (parser, names of the flags that are accepted and ignored)"""
    from rotate_yolov3_amd.utils.cli import add_ignored
    parser = argparse.ArgumentParser(prog='test.py')                   # the reference's flags (test.py:206-216), same defaults
    parser.add_argument('--hyp', type=str, default='cfg/ICDAR/hyp.py', help='hyper-parameter path')
    parser.add_argument('--cfg', type=str, default='cfg/ICDAR/yolov3_608_se.cfg', help='cfg file path')
    parser.add_argument('--data', type=str, default='data/icdar_13+15.data', help='*.data file path (`classes`; with --real-data also `valid`, the image list)')
    parser.add_argument('--weights', type=str, default='weights/best.pt', help='path to weights file (.pt or darknet .weights)')
    parser.add_argument('--batch-size', type=int, default=1, help='size of each image batch')
    parser.add_argument('--img-size', type=int, default=608, help='inference size (pixels)')
    parser.add_argument('--iou-thres', type=float, default=0.5, help='iou threshold required to qualify as detected')
    parser.add_argument('--conf-thres', type=float, default=0.001, help='object confidence threshold')
    parser.add_argument('--nms-thres', type=float, default=0.5, help='iou threshold for non-maximum suppression')
    parser.add_argument('--device', default='', help="device id (i.e. 0 or 0,1); the evaluation path has no CPU fallback")
    parser.add_argument('--synthetic', type=int, default=32, help='synthetic images to evaluate (without --real-data)')
    parser.add_argument('--real-data', action='store_true', help='evaluate the `valid` image list of --data instead of synthetic images (needs Pillow)')
    parser.add_argument('--nms-style', type=str, default='OR', choices=['OR', 'MERGE'], help='OR: greedy rotated NMS; MERGE: every kept box becomes the score-weighted mean of the boxes it suppresses')
    ignored = add_ignored(parser, [('--save-json', dict(action='store_true', help='save a cocoapi-compatible JSON results file'))])
    return parser, ignored


if __name__ == '__main__':
    from rotate_yolov3_amd.utils.cli import pick_device, report_ignored
    from rotate_yolov3_amd.utils.parse_config import parse_data_cfg
    parser, ignored = build_parser()
    opt = parser.parse_args()
    print(opt)
    report_ignored(parser, opt, ignored)
    device = pick_device(opt.device)
    if device.type != 'cuda':
        sys.exit('test.py: the evaluation path (HIP forward, rotated NMS, rotated-IoU matching) needs a GPU; --device %r selects none' % opt.device)
    weights = opt.weights if os.path.isfile(opt.weights) else ''
    if opt.weights and not weights:
        print('NOTE: weights file %r not found: evaluating the freshly initialised model' % opt.weights)
    loader = None
    if opt.real_data:
        from rotate_yolov3_amd.utils.datasets import LoadImagesAndLabels
        loader = LoadImagesAndLabels(parse_data_cfg(opt.data)['valid'], opt.img_size, opt.batch_size, augment=False, device=device)
    test(opt.cfg, hyp_parse(opt.hyp), weights, opt.batch_size, opt.img_size, opt.iou_thres, opt.conf_thres, opt.nms_thres,
         n_images=opt.synthetic, device=device,
         nc=int(parse_data_cfg(opt.data)['classes']) if os.path.isfile(opt.data) else None, loader=loader, nms_style=opt.nms_style)
