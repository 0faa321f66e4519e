#!/usr/bin/env python
"""Time the detection input path two ways, per batch of `--bs` procedurally generated 2048 x 1536 images, to 608 x 608 and to three scales:
  (a) host resize: what the tree offered before ryolo_letterbox_area -- per image and per scale Pillow Image.BOX to letterbox's new_unpad,
      upload of the reduced pixels, ryolo_letterbox_augment with neutral parameters;
  (b) device resize: ONE upload of the original pixels, ryolo_letterbox_area per scale.
Host clock around work that ends in a device synchronise (both include their uploads; decoding is outside both), after a warm-up, median
of `--repeats`, the two alternating.  Then the kernel alone at ratio 1 beside ryolo_letterbox_augment neutral at the same shape (bs 64,
608 x 608, sources of exactly the placed size), and the kernel alone at the detection ratio: device events around back-to-back launches.
Prints the table kept as profiles/detect_input.txt.
    python tools/detect_input_time.py [--bs 8] [--repeats 7] [--iters 50] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.model import hip_ops as ops  # noqa: E402
from rotate_yolov3_amd.utils import datasets as ds  # noqa: E402


def picture(h, w, seed):
    """smooth colour waves plus noise: compresses like nothing, resamples like a photograph"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([127 + 100 * np.sin(x / (40 + seed) + y / 90), 127 + 100 * np.cos(x / 23 - y / (31 + seed)), 127 + 100 * np.sin(y / 17)], 2)
    return np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters       # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", type=str, default="")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from PIL import Image
    dev = torch.device("cuda:0")
    bs, H0, W0 = opt.bs, 1536, 2048
    arrays = [picture(H0, W0, i) for i in range(bs)]
    pil = [Image.fromarray(a) for a in arrays]
    shapes = [(H0, W0)] * bs
    lines = []

    def host_path(sizes):
        for S in sizes:
            small = [np.asarray(im.resize(ds.letterbox_matrix(H0, W0, S).new_unpad, Image.BOX), dtype=np.uint8) for im in pil]
            cache = ds.DeviceImageCache.from_arrays(small, dev)
            rows = np.stack([ds.param_row(ds.NEUTRAL, *cache.hw[i], S, cache.maxima[i]) for i in range(bs)])
            ops.letterbox_augment(cache, torch.arange(bs, dtype=torch.int32).to(dev), torch.from_numpy(rows).to(dev), 0, S, S)
        torch.cuda.synchronize()

    def device_path(sizes):
        cache = ds.DeviceImageCache.from_arrays(arrays, dev)
        for S in sizes:
            ds.letterbox_batch(cache, shapes, S)
        torch.cuda.synchronize()

    def clock(fn, sizes):
        t0 = time.perf_counter()
        fn(sizes)
        return (time.perf_counter() - t0) * 1e3

    lines.append("library %s; %d images of %d x %d uint8 RGB (%.1f MB); host threads %d"
                 % (_lib.lib().ryolo_build_id().decode(), bs, W0, H0, bs * H0 * W0 * 3 / 1e6, torch.get_num_threads()))
    lines.append("milliseconds per batch, host clock to a device synchronise, median of %d (min .. max); uploads included, decoding not"
                 % opt.repeats)
    for sizes in ((608,), (416, 608, 800)):
        for fn in (host_path, device_path):
            clock(fn, sizes)
        t = {host_path: [], device_path: []}
        for _ in range(opt.repeats):
            for fn in (host_path, device_path):
                t[fn].append(clock(fn, sizes))
        for fn, name in ((host_path, "(a) Pillow BOX per image and scale + upload + ryolo_letterbox_augment neutral"),
                         (device_path, "(b) one upload of the originals + ryolo_letterbox_area per scale")):
            lines.append("  to %-14s %-80s %8.2f  (%.2f .. %.2f)" % ("x".join(str(s) for s in sizes), name, float(np.median(t[fn])),
                                                                      min(t[fn]), max(t[fn])))

    # the kernels alone
    cache = ds.DeviceImageCache.from_arrays(arrays, dev)
    src = torch.arange(bs, dtype=torch.int32, device=dev)
    calls = {}
    for S in (416, 608, 800):
        out = torch.empty((bs, S, S, 8), dtype=torch.bfloat16, device=dev)
        place = ds.place_rows(shapes, S)
        calls["ryolo_letterbox_area, bs %d, %d x %d -> %d^2 (ratio %.2f)" % (bs, W0, H0, S, W0 / S)] = \
            (lambda S=S, out=out, place=place: ops.letterbox_area(cache, src, place, S, S, out=out))
    n1, S1 = 64, 608
    rng = np.random.default_rng(0)
    same = []
    for i in range(n1):
        short = int(rng.integers(S1 // 2, S1 + 1))
        h, w = (S1, short) if i % 3 == 0 else (short, S1)
        same.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    cache1 = ds.DeviceImageCache.from_arrays(same, dev)
    src1 = torch.arange(n1, dtype=torch.int32, device=dev)
    out1 = torch.empty((n1, S1, S1, 8), dtype=torch.bfloat16, device=dev)
    place1 = ds.place_rows(cache1.hw, S1)
    rows1 = torch.from_numpy(np.stack([ds.param_row(ds.NEUTRAL, *cache1.hw[i], S1, cache1.maxima[i]) for i in range(n1)])).to(dev)
    calls["ryolo_letterbox_area, bs 64, 608^2, ratio 1 (sources of the placed size)"] = \
        lambda: ops.letterbox_area(cache1, src1, place1, S1, S1, out=out1)
    calls["ryolo_letterbox_augment neutral, the same batch"] = lambda: ops.letterbox_augment(cache1, src1, rows1, 0, S1, S1, out=out1)
    for fn in calls.values():
        events(fn, 5)
    times = {k: [] for k in calls}
    for _ in range(5):
        for k, fn in calls.items():
            times[k].append(events(fn, opt.iters))
    lines.append("microseconds per call (wrapper + launch): device events around %d back-to-back calls, median of 5 (min .. max)" % opt.iters)
    for k, v in times.items():
        lines.append("  %-80s %8.1f  (%.1f .. %.1f)" % (k, float(np.median(v)), min(v), max(v)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
