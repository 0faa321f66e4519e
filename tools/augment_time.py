#!/usr/bin/env python
"""Time ryolo_letterbox_augment beside ryolo_nchw_f32_to_nhwc_bf16 (the pass it replaces at the model boundary) at the training shape:
bs 64, 608 x 608, from a cache of 64 seeded uint8 images of HRSC-like sizes.  Device events around `--iters` back-to-back launches after
a warm-up, five repeats each, the configurations interleaved; prints the table kept as profiles/augment.txt.
    python tools/augment_time.py [--bs 64] [--size 608] [--iters 50]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.model import hip_ops as ops  # noqa: E402
from rotate_yolov3_amd.utils import datasets as ds  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters       # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--iters", type=int, default=50)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    bs, S = opt.bs, opt.size
    rng = np.random.default_rng(0)
    images = []
    for i in range(bs):
        short = int(rng.integers(S // 2, S + 1))
        h, w = (S, short) if i % 3 == 0 else (short, S)
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    cache = ds.DeviceImageCache.from_arrays(images, dev)
    hyp = dict(degrees=10.0, translate=0.1, scale=0.2, noise=0.03, gamma=0.3, blur=1.3, hsv_s=0.5, hsv_v=0.4, grayscale=0.3)
    everything = {k: 1.0 for k in ds.PROBS}
    full = [ds.draw_params(hyp, ds.draw_rng(0, 0, i), probs=everything) for i in range(bs)]
    configs = {
        "letterbox only (augment=False)": [ds.NEUTRAL] * bs,
        "affine + flips": [ds.NEUTRAL._replace(affine=d.affine, hflip=d.hflip, vflip=d.vflip) for d in full],
        "every stage but blur": [d._replace(blur_sigma=0.0) for d in full],
        "every stage (blur: the LDS path)": full,
        "training mix (the reference's probabilities)": [ds.draw_params(hyp, ds.draw_rng(0, 0, i)) for i in range(bs)],
    }
    src = torch.arange(bs, dtype=torch.int32, device=dev)
    out = torch.empty((bs, S, S, 8), dtype=torch.bfloat16, device=dev)
    calls = {}
    for name, draws in configs.items():
        rows = torch.from_numpy(np.stack([ds.param_row(d, *cache.hw[i], S, cache.maxima[i]) for i, d in enumerate(draws)])).to(dev)
        calls[name] = (lambda rows=rows: ops.letterbox_augment(cache, src, rows, 1, S, S, out=out))
    x32 = torch.rand(bs, 3, S, S, device=dev)
    calls["ryolo_nchw_f32_to_nhwc_bf16 (fp32 batch already on the device)"] = lambda: ops.nchw_f32_to_nhwc_bf16(x32)
    for fn in calls.values():
        timed(fn, 5)
    times = {k: [] for k in calls}
    for _ in range(5):
        for k, fn in calls.items():
            times[k].append(timed(fn, opt.iters))
    print("library %s; bs %d, %d x %d, cache %.1f MB of uint8 in %d images; output %.1f MB of bf16 [N, H, W, 8]"
          % (_lib.lib().ryolo_build_id().decode(), bs, S, S, cache.nbytes / 1e6, cache.n, out.numel() * 2 / 1e6))
    print("microseconds per launch: device events around %d back-to-back launches, median of 5 (min .. max)" % opt.iters)
    for k, v in times.items():
        print("  %-68s %8.1f  (%.1f .. %.1f)" % (k, float(np.median(v)), min(v), max(v)))


if __name__ == "__main__":
    main()
