"""Oracle of csrc/draw.hip and of ryolo_det_corners, restated with numpy int64 (no cv2): the definition of include/ryolo.h, nothing of
the kernel's tiling.  At the test sizes every product stays below 2^63.

corners(det)                       ryolo_det_corners: np.trunc(rotated_corners(det[:, :5])) -> (int64 [M, 8], the float64 they came from)
covers(quad, t, h, w)              bool [h, w]: the pixels whose distance to one of the four closed edges has 4 dist^2 <= t^2
draw(pixels, offsets, hw, ...)     ryolo_draw_quads on a flat uint8 array: per pixel the colour of the LARGEST covering row of its image"""
import numpy as np

from rotate_yolov3_amd.utils.datasets import rotated_corners

COORD_MIN, COORD_MAX = -16384, 32767


def corners(det):
    det = np.asarray(det, dtype=np.float64).reshape(-1, 8)
    xy = rotated_corners(det[:, :5])
    return np.trunc(xy).astype(np.int64), xy


def in_range(quad):
    q = np.asarray(quad, dtype=np.int64).reshape(8)
    return bool((q >= COORD_MIN).all() and (q <= COORD_MAX).all())


def covers(quad, t, h, w):
    """the outline of one row on an h x w image (no range rule here: see draw)"""
    q = np.asarray(quad, dtype=np.int64).reshape(4, 2)
    t2 = int(t) * int(t)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.zeros((h, w), dtype=bool)
    for k in range(4):
        (ax, ay), (bx, by) = q[k], q[(k + 1) % 4]
        dx, dy = bx - ax, by - ay
        L2 = dx * dx + dy * dy
        ex, ey = x - ax, y - ay
        u = ex * dx + ey * dy
        near_a = 4 * (ex * ex + ey * ey) <= t2
        near_b = 4 * ((x - bx) ** 2 + (y - by) ** 2) <= t2
        c = ex * dy - ey * dx
        c2 = 2 * np.abs(c)                               # 4 c^2 <= t^2 L2 < 2^49: false from 2 |c| = 2^32 on, below that (2 |c|)^2 < 2^64
        big = c2 >= 1 << 32
        c2 = np.where(big, 0, c2).astype(np.uint64)
        between = ~big & (c2 * c2 <= np.uint64(t2 * int(L2)))
        out |= np.where((u <= 0) | (L2 == 0), near_a, np.where(u >= L2, near_b, between))
    return out


def label_covers(bits, off, rect, h, w):
    """the label of one row: rect = (lx, ly, lw, lh), one byte per label pixel from bits[off]"""
    lx, ly, lw, lh = (int(v) for v in rect)
    out = np.zeros((h, w), dtype=bool)
    if lw <= 0 or lh <= 0:
        return out
    bm = np.asarray(bits[int(off):int(off) + lw * lh]).reshape(lh, lw) != 0
    x0, y0, x1, y1 = max(lx, 0), max(ly, 0), min(lx + lw, w), min(ly + lh, h)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = bm[y0 - ly:y1 - ly, x0 - lx:x1 - lx]
    return out


def draw_image(img, quads, colors, t, labels=None):
    """one image [h, w, 3]: rows in order, a later row paints over an earlier one -- the largest covering row wins"""
    out = np.array(img, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    for r in range(len(quads)):
        if not in_range(quads[r]):
            continue                                     # neither outline nor label
        m = covers(quads[r], t, h, w)
        if labels is not None:
            m |= label_covers(labels[0], labels[1][r], labels[2][r], h, w)
        out[m] = np.asarray(colors[r], dtype=np.uint8)[:3]
    return out


def draw(pixels, offsets, hw, quad, det_off, color, thick, labels=None, dst=None):
    """-> the flat uint8 array ryolo_draw_quads leaves in dst (a copy of `dst` to start from: the bytes outside the images keep its values;
    None: pixels itself).  labels: None or (lab_bits, lab_off [M], lab_rect [M, 4])"""
    pixels = np.asarray(pixels, dtype=np.uint8)
    out = np.array(pixels if dst is None else dst, dtype=np.uint8, copy=True)
    quad = np.asarray(quad, dtype=np.int64).reshape(-1, 8)
    for b, (h, w) in enumerate(hw):
        o = int(offsets[b])
        lo, hi = (int(det_off[b]), int(det_off[b + 1])) if len(quad) else (0, 0)
        lab = None if labels is None else (labels[0], np.asarray(labels[1])[lo:hi], np.asarray(labels[2])[lo:hi])
        img = draw_image(pixels[o:o + 3 * h * w].reshape(h, w, 3), quad[lo:hi], np.asarray(color)[lo:hi], int(thick[b]), lab)
        out[o:o + 3 * h * w] = img.reshape(-1)
    return out
