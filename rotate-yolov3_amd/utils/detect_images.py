"""Detection on cached images: single-scale detect() and multi_detect() of the reference's detect.py (:16-137, :142-275) for a whole batch.

Per network size: ryolo_letterbox_area from the original pixels, Darknet.detect (forward + rotated NMS), ryolo_det_rescale on the flat
rows -- scale_coords(...).round().  With one size that is the result.  With several, each size's NMS runs at scale_nms_thres (0.95 in the
reference: near-duplicates only), every image's rows are concatenated in (image, scale, row) order, the reference's filters are applied
again to the rescaled rows (score > conf_thres, w and h > 2, finite) and ONE segmented rotated NMS at nms_thres merges them.

The scores are taken as they are.  The reference feeds its 8-column rows (x, y, w, h, a, score, class_conf, class) back into
non_max_suppression, which reads columns 6.. as class scores: for a one-class model (class_conf 1, class 0) that is the same thing; for
more classes it multiplies the score by max(class_conf, class index) and renumbers the classes 0 / 1 -- an accident that is not kept."""
import numpy as np
import torch

from ..model import hip_ops
from .datasets import letterbox_batch
from .nms.nms import _flat, check_nms_style, nms_from_candidates


def rescale_geometry(shapes, size):
    """fp32 [n, 3] rows (gain, pad_x, pad_y) of scale_coords for (h0, w0) images letterboxed into size x size: computed in double"""
    g = np.empty((len(shapes), 3), dtype=np.float64)
    for k, (h0, w0) in enumerate(shapes):
        gain = float(size) / max(h0, w0)
        g[k] = (gain, (size - w0 * gain) / 2, (size - h0 * gain) / 2)
    return g.astype(np.float32)


def _split(det, det_off, n):
    off = det_off.tolist()
    return [det[off[b]:off[b + 1]] if off[b + 1] > off[b] else None for b in range(n)]


def detect_images(model, cache, n, shapes, img_sizes, conf_thres, nms_thres, scale_nms_thres=0.95, slots=None, nms_style='OR'):
    """-> (output, det, det_off): list[n] of [k, 8] rows (x, y, w, h, a, score, class_conf, class) in ORIGINAL image pixels, rounded, by
    descending score (None: no detection); the same rows back to back, fp32 [M, 8]; their offsets, int32 [n + 1] on the device.
    cache: the device cache of the n images, shapes their (h, w); img_sizes: the network sizes; slots >= n: the engine's batch size (the
    slots past n are border and their rows are dropped).
    nms_style 'MERGE' (utils/nms/nms.py): with one size, that size's NMS; with several, the final NMS over the scales alone -- the
    same object found at several sizes gives several estimates of one box, and the kept row becomes their score-weighted mean (not
    rounded again); the per-size passes at scale_nms_thres only remove duplicates inside a scale and stay 'OR'."""
    check_nms_style(nms_style)
    shapes = [tuple(int(v) for v in s) for s in shapes][:n]
    if len(shapes) != n or not img_sizes:
        raise ValueError("detect_images: %d shapes for %d images, sizes %r" % (len(shapes), n, list(img_sizes)))
    dev = cache.pixels.device
    multi = len(img_sizes) > 1
    rows, imgs = [], []
    with torch.no_grad():
        for size in img_sizes:
            batch = letterbox_batch(cache, shapes, int(size), slots)
            if multi or nms_style == 'OR':
                out = model.detect(batch, conf_thres, scale_nms_thres if multi else nms_thres)[:n]
            else:
                out = model.detect(batch, conf_thres, nms_thres, nms_style=nms_style)[:n]
            det, det_off = _flat(out, dev)
            hip_ops.det_rescale(det, det_off, torch.from_numpy(rescale_geometry(shapes, size)).to(dev))
            if not multi:
                return _split(det, det_off, n), det, det_off
            rows.append(det)
            counts = (det_off[1:] - det_off[:-1]).long()
            imgs.append(torch.repeat_interleave(torch.arange(n, device=dev), counts))
        cand, img = torch.cat(rows), torch.cat(imgs)
        o = img.argsort(stable=True)                      # (image, scale, row)
        cand, img = cand[o], img[o]
        ok = (cand[:, 5] > conf_thres) & (cand[:, 2:4] > 2).all(1) & torch.isfinite(cand).all(1)
        cand, img = cand[ok], img[ok]
        if cand.shape[0] == 0:
            return [None] * n, torch.zeros(0, 8, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev)
        return nms_from_candidates(img, cand, n, nms_thres, flat=True, nms_style=nms_style)
