"""mAP matching of one evaluation batch: the per-image loop (metrics.match_predictions, one IoU-matrix launch, three host copies and a
Python walk per image) against the batched call (metrics.match_predictions_batched -> ryolo_eval_match, three launches per batch).

    python tools/eval_match_bench.py [--images 16] [--preds 4096] [--labels 32] [--out profiles/eval_match.txt]

Load: `images` images x `preds` predictions x `labels` labels, 3 classes -- test.py at --conf-thres 0.001.  A fifth of the predictions are
jittered copies of labels (a fifth of those with a wrong class), the rest background from synthetic.random_boxes; score-descending per
image.  One process, one device, profiler off.  Three figures, each the median of `--rounds` rounds with the spread, the two host-side
paths alternating inside a round, after a warm-up round of both:
  loop      wall time of the per-image loop over the batch (it ends in host copies, so it is synchronous)
  batched   wall time of match_predictions_batched up to a final device synchronise
  device    HIP events around ryolo_eval_match's three launches alone (the C ABI called directly, buffers allocated beforehand)
and the two results are compared flag for flag before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.utils import metrics  # noqa: E402
from rotate_yolov3_amd.utils.synthetic import random_boxes  # noqa: E402


def make_load(n_img, n_pred, n_lab, classes=3, seed=0):
    """(det [n_img * n_pred, 8], det_off, targets_px [n_img * n_lab, 7]) as numpy arrays"""
    r = np.random.RandomState(seed)
    dets, tgts = [], []
    for im in range(n_img):
        lab = np.zeros((n_lab, 7), dtype=np.float32)
        lab[:, 0] = im
        lab[:, 1] = r.randint(0, classes, n_lab)
        lab[:, 2:4] = r.uniform(60, 548, (n_lab, 2))
        lab[:, 4] = r.uniform(60, 160, n_lab)
        lab[:, 5] = lab[:, 4] / r.uniform(3, 8, n_lab)
        lab[:, 6] = r.uniform(-1.5, 1.5, n_lab)
        pred = np.zeros((n_pred, 8), dtype=np.float32)
        pred[:, :6] = random_boxes(n_pred, seed=seed * 1000 + im)
        pred[:, 6] = 1.0
        pred[:, 7] = r.randint(0, classes, n_pred)
        near = n_pred // 5
        src = lab[r.randint(0, n_lab, near)]
        pred[:near, :5] = src[:, 2:7] + r.normal(0, 1, (near, 5)) * np.array([6, 6, 8, 3, 0.08]) * r.choice([0.15, 0.4, 1.2], (near, 1))
        pred[:near, 7] = np.where(r.rand(near) < 0.8, src[:, 1], (src[:, 1] + 1) % classes)
        dets.append(pred[np.argsort(-pred[:, 5], kind="stable")])
        tgts.append(lab)
    det_off = np.arange(n_img + 1, dtype=np.int32) * n_pred
    return np.concatenate(dets), det_off, np.concatenate(tgts)


def med(xs):
    m = statistics.median(xs)
    return m, 100.0 * (max(xs) - min(xs)) / (2 * m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--preds", type=int, default=4096)
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iou-thres", type=float, default=0.5)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "eval_match_bench measures on the GPU: there is no CPU path"
    dev = torch.device("cuda:0")
    det_h, off_h, tgt_h = make_load(opt.images, opt.preds, opt.labels)
    det, det_off, tgt = [torch.from_numpy(a).to(dev) for a in (det_h, off_h, tgt_h)]
    n_img, thr = opt.images, opt.iou_thres
    per_image = [(det[off_h[k]:off_h[k + 1]], tgt[tgt[:, 0] == k, 1:].contiguous()) for k in range(n_img)]

    def loop():
        out = []
        for p, t in per_image:
            out += metrics.match_predictions(p, t, thr)
        return out

    def batched():
        c, _ = metrics.match_predictions_batched(det, det_off, tgt, n_img, thr)
        torch.cuda.synchronize(dev)
        return c

    want, got = loop(), batched().cpu().tolist()
    assert want == got, "the batched matcher and the per-image loop disagree"
    # the C ABI alone, for the device time of the three launches
    L = _lib.lib()
    lab = tgt[:, 1:7].contiguous()
    lab_off = torch.arange(n_img + 1, dtype=torch.int32, device=dev) * opt.labels
    correct = torch.empty(len(det), dtype=torch.uint8, device=dev)
    matched = torch.empty(len(det), dtype=torch.int32, device=dev)
    ws = torch.empty(L.ryolo_eval_match_workspace_bytes(len(det), len(lab)), dtype=torch.uint8, device=dev)

    def launches():
        rc = L.ryolo_eval_match(det.data_ptr(), 8, det_off.data_ptr(), lab.data_ptr(), 6, lab_off.data_ptr(), n_img, len(det), len(lab),
                                thr, correct.data_ptr(), matched.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
        assert rc == 0, rc

    launches()
    torch.cuda.synchronize(dev)
    assert correct.cpu().tolist() == want
    t_loop, t_batched, t_dev = [], [], []
    for rnd in range(opt.rounds + 1):                      # round 0 warms both paths up and is dropped
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        loop()
        t1 = time.perf_counter()
        reps = 20
        for _ in range(reps):
            batched()
        t2 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launches()
        e1.record()
        torch.cuda.synchronize(dev)
        if rnd:
            t_loop.append((t1 - t0) * 1e3)
            t_batched.append((t2 - t1) * 1e3 / reps)
            t_dev.append(e0.elapsed_time(e1) / reps)
    (ml, sl), (mb, sb), (md, sd) = med(t_loop), med(t_batched), med(t_dev)
    n_correct = int(np.sum(want))
    lines = [
        "# mAP matching of one evaluation batch: per-image loop vs ryolo_eval_match (csrc/skewiou.hip), one MI355X, one process",
        "# python tools/eval_match_bench.py --out ...      (profiler off)",
        "",
        "eval_match_bench: %d images x %d predictions x %d labels, 3 classes, iou_thres %.2f, %s, library %s"
        % (n_img, opt.preds, opt.labels, thr, torch.cuda.get_device_name(dev), L.ryolo_build_id().decode()),
        "%d predictions, %d correct; the two paths agree flag for flag" % (len(det), n_correct),
        "median of %d rounds after one warm-up round (spread = half the range); batched and device: 20 calls per round" % opt.rounds,
        "per-image loop (match_predictions x %d), host wall        %10.3f ms  (+-%.1f %%)" % (n_img, ml, sl),
        "batched call (match_predictions_batched), host wall to sync %8.3f ms  (+-%.1f %%)" % (mb, sb),
        "ryolo_eval_match's three launches, HIP events               %8.3f ms  (+-%.1f %%)" % (md, sd),
        "loop / batched = %.1f" % (ml / mb),
        "The batched call is %s than the loop it replaces at this load." % ("FASTER" if mb < ml else "NOT faster"),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
