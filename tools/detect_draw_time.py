#!/usr/bin/env python
"""Time drawing the detections into a batch of `--bs` procedurally generated 2048 x 1536 images two ways, with 10, 100 and 1000 boxes per
image (outline of thickness line_thickness(h, w) plus a label each):
  (a) host drawing: what the tree could do without ryolo_draw_quads -- download the original pixels, then per box Pillow
      ImageDraw.line(width=t) around the four corners plus ImageDraw.text;
  (b) device drawing: utils.plots.draw_detections (ryolo_det_corners + ryolo_draw_quads, label bitmaps from the cache), then ONE download.
Host clock around work that ends in a device synchronise, after a warm-up, median of `--repeats`, the two alternating, the profiler off.
Encoding (PNG and JPEG at quality 95, one thread and the pool of 8) is timed separately: both ways pay it alike.  Then ryolo_draw_quads
alone: device events around `--iters` back-to-back calls.  Prints the table kept as profiles/detect_draw.txt.
    python tools/detect_draw_time.py [--bs 8] [--repeats 7] [--iters 50] [--out FILE]"""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.model import hip_ops as ops  # noqa: E402
from rotate_yolov3_amd.utils import datasets as ds  # noqa: E402
from rotate_yolov3_amd.utils import plots  # noqa: E402
from tools.detect_input_time import events, picture  # noqa: E402


def boxes(n_img, per_image, h, w, seed):
    """fp32 [n_img * per_image, 8] rows like detect.py's: integer centres and sizes (text-line shaped: 40..400 x 12..80), any angle"""
    rng = np.random.default_rng(seed)
    m = n_img * per_image
    det = np.zeros((m, 8), dtype=np.float32)
    det[:, 0], det[:, 1] = rng.integers(0, w, m), rng.integers(0, h, m)
    det[:, 2], det[:, 3] = rng.integers(40, 400, m), rng.integers(12, 80, m)
    det[:, 4] = rng.uniform(-np.pi / 2, np.pi / 2, m)
    det[:, 5] = rng.uniform(0.3, 1.0, m)
    det[:, 6] = 1.0
    return det, np.arange(0, m + 1, per_image, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", type=str, default="")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from PIL import Image, ImageDraw
    dev = torch.device("cuda:0")
    bs, H0, W0 = opt.bs, 1536, 2048
    arrays = [picture(H0, W0, i) for i in range(bs)]
    cache = ds.DeviceImageCache.from_arrays(arrays, dev)
    t = plots.line_thickness(H0, W0)
    colors = plots.class_colors(plots.DEFAULT_CLASSES)
    size = max(10, 7 * t)
    font = plots._font(size)
    lines = []

    def host_path(det, off):
        flat = cache.pixels.cpu().numpy()                 # the download ends in a synchronise
        corners = np.trunc(ds.rotated_corners(det[:, :5])).astype(np.int64).reshape(-1, 4, 2)
        out = []
        for b in range(bs):
            im = Image.fromarray(flat[b * H0 * W0 * 3:(b + 1) * H0 * W0 * 3].reshape(H0, W0, 3))
            d = ImageDraw.Draw(im)
            for r in range(off[b], off[b + 1]):
                c = tuple(int(v) for v in colors[int(det[r, 7]) % len(colors)])
                q = [tuple(p) for p in corners[r].tolist()]
                d.line(q + q[:1], fill=c, width=t)
                d.text((q[0][0], q[0][1] - size), plots.label_text(None, det[r, 7], det[r, 5]), fill=c, font=font)
            out.append(im)
        return out

    def device_path(det_t, off_t, rows):
        drawn = plots.draw_detections(cache, bs, det_t, off_t, None, colors, host_rows=rows).cpu().numpy()
        return [drawn[b * H0 * W0 * 3:(b + 1) * H0 * W0 * 3].reshape(H0, W0, 3) for b in range(bs)]

    def clock(fn, *a):
        t0 = time.perf_counter()
        r = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    lines.append("library %s; %d images of %d x %d uint8 RGB (%.1f MB); thickness %d, label font size %d; host threads %d"
                 % (_lib.lib().ryolo_build_id().decode(), bs, W0, H0, bs * H0 * W0 * 3 / 1e6, t, size, torch.get_num_threads()))
    lines.append("milliseconds per batch, host clock to a device synchronise, median of %d (min .. max); the download included, encoding not"
                 % opt.repeats)
    kernel_calls = {}
    last = None
    for per_image in (10, 100, 1000):
        det, off = boxes(bs, per_image, H0, W0, per_image)
        det_t, off_t, rows = torch.from_numpy(det).to(dev), torch.from_numpy(off).to(dev), det.tolist()
        clock(host_path, det, off)
        clock(device_path, det_t, off_t, rows)            # warm: the label cache holds every text from here on
        ta, tb = [], []
        for _ in range(opt.repeats):
            ta.append(clock(host_path, det, off)[0])
            ms, last = clock(device_path, det_t, off_t, rows)
            tb.append(ms)
        for name, v in (("(a) download + Pillow ImageDraw.line(width=%d) + text per box" % t, ta),
                        ("(b) draw_detections (ryolo_det_corners + ryolo_draw_quads) + one download", tb)):
            lines.append("  %5d boxes per image  %-78s %9.2f  (%.2f .. %.2f)" % (per_image, name, float(np.median(v)), min(v), max(v)))
            print(lines[-1], file=sys.stderr, flush=True)
        quad = ops.det_corners(det_t)
        color = torch.zeros(len(det), 4, dtype=torch.uint8, device=dev)
        labels = plots.pack_labels([plots.render_label(plots.label_text(None, r[7], r[5]), t) for r in rows], quad[:, :2])
        out = torch.empty_like(cache.pixels)
        kernel_calls["ryolo_draw_quads, %d x %d boxes, outlines + labels, out of place" % (bs, per_image)] = \
            (lambda quad=quad, off_t=off_t, color=color, labels=labels, out=out: ops.draw_quads(cache, quad, off_t, color, t, labels=labels, out=out))
        kernel_calls["ryolo_draw_quads, %d x %d boxes, outlines only, out of place" % (bs, per_image)] = \
            (lambda quad=quad, off_t=off_t, color=color, out=out: ops.draw_quads(cache, quad, off_t, color, t, out=out))
        work = cache.pixels.clone()
        kernel_calls["ryolo_draw_quads, %d x %d boxes, outlines + labels, in place" % (bs, per_image)] = \
            (lambda quad=quad, off_t=off_t, color=color, labels=labels, work=work:
             ops.draw_quads((work, cache.img_offset, cache.img_hw, cache.hw), quad, off_t, color, t, labels=labels, out=work))

    # encoding: the same for both ways
    def encode(a, fmt):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format=fmt, **({"quality": 95} if fmt == "JPEG" else {}))
        return buf.tell()

    lines.append("encoding the %d drawn images (1000 boxes each) to memory, milliseconds per batch, median of %d (min .. max)" % (bs, opt.repeats))
    for fmt in ("JPEG", "PNG"):
        for workers in (1, 8):
            v = []
            for _ in range(opt.repeats):
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=workers) as pool:
                    sizes = list(pool.map(lambda a: encode(a, fmt), last))
                v.append((time.perf_counter() - t0) * 1e3)
            lines.append("  %-4s %d thread%s  %9.2f  (%.2f .. %.2f)   %.1f MB" % (fmt, workers, " " if workers == 1 else "s", float(np.median(v)),
                                                                                 min(v), max(v), sum(sizes) / 1e6))
            print(lines[-1], file=sys.stderr, flush=True)

    for fn in kernel_calls.values():
        events(fn, 3)
    times = {k: [] for k in kernel_calls}
    for _ in range(5):
        for k, fn in kernel_calls.items():
            times[k].append(events(fn, opt.iters))
    lines.append("microseconds per call (wrapper + launch): device events around %d back-to-back calls, median of 5 (min .. max); %.1f MB read, "
                 "as much written out of place" % (opt.iters, cache.nbytes / 1e6))
    for k, v in times.items():
        lines.append("  %-78s %9.1f  (%.1f .. %.1f)" % (k, float(np.median(v)), min(v), max(v)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
