"""Oracles of csrc/detpost.hip, restated with numpy (no cv2, no scipy):

rescale(det, det_off, geom)   ryolo_det_rescale in numpy float32 -- IEEE subtract / divide and np.rint (round half to even, like rintf):
                              scale_coords(...).round() of the reference (utils/utils.py:181-189) with the gain and the paddings of
                              utils.detect_images.rescale_geometry.
quads(det)                    ryolo_det_quads in float64: xywha2icdar of the reference (utils/ICDAR/icdar_utils.py:105-135) with the corners
                              of utils.datasets.rotated_corners and order_points made deterministic (stable sorts; of the two right-most
                              corners the one farther from tl is br, on a tie the later one).  Returns the int64 rows and the float64
                              coordinates they were truncated from."""
import numpy as np

from rotate_yolov3_amd.utils.datasets import rotated_corners


def rescale(det, det_off, geom):
    out = np.array(det, dtype=np.float32, copy=True).reshape(-1, 8)
    geom = np.asarray(geom, dtype=np.float32)
    for b in range(len(det_off) - 1):
        r = slice(int(det_off[b]), int(det_off[b + 1]))
        gain, px, py = geom[b]
        out[r, 0] = np.rint((out[r, 0] - px) / gain)
        out[r, 1] = np.rint((out[r, 1] - py) / gain)
        out[r, 2] = np.rint(out[r, 2] / gain)
        out[r, 3] = np.rint(out[r, 3] / gain)
    assert out.dtype == np.float32
    return out


def order_points(pts):
    """[4, 2] corners -> [4, 2] in tl, tr, br, bl order"""
    xs = pts[np.argsort(pts[:, 0], kind='stable')]
    left, right = xs[:2], xs[2:]
    tl, bl = left[np.argsort(left[:, 1], kind='stable')]
    d = ((right - tl) ** 2).sum(1)                       # squared distances order like cdist's
    br, tr = right[np.argsort(d, kind='stable')[::-1]]
    return np.stack([tl, tr, br, bl])


def quad_boxes(seed=11, n=300, extent=2048):
    """fp32 [n, 8] detection rows for the ryolo_det_quads tests: integer x, y, w, h as the rescale leaves them (w, h > 2), angles random
    in (-pi/2, pi/2) but for ten rows each at exactly 0, +fp32(pi/2) and -fp32(pi/2), where order_points meets ties and near-ties"""
    rng = np.random.default_rng(seed)
    det = np.zeros((n, 8), dtype=np.float32)
    det[:, 0:2] = rng.integers(0, extent, (n, 2))
    det[:, 2:4] = rng.integers(3, 400, (n, 2))
    det[:, 4] = rng.uniform(-np.pi / 2, np.pi / 2, n).astype(np.float32).clip(-1.5707, 1.5707)
    det[0:10, 4] = 0.0
    det[10:20, 4] = np.float32(np.pi / 2)
    det[20:30, 4] = -np.float32(np.pi / 2)
    det[:, 5] = rng.uniform(0, 1, n)
    det[:, 6] = 1.0
    return det


def comparable(det, margin=1e-6):
    """mask of the rows whose every oracle coordinate is farther than `margin` from an integer (truncation there would hang on the last
    bits of the device's cos / sin), or whose angle is exactly 0, where the arithmetic is exact"""
    _, xy = quads(det)
    return (np.abs(xy - np.rint(xy)) > margin).all(1) | (np.asarray(det)[:, 4] == 0)


def quads(det):
    det = np.asarray(det, dtype=np.float64).reshape(-1, 8)
    corners = rotated_corners(det[:, :5]).reshape(-1, 4, 2)
    ordered = np.stack([order_points(c) for c in corners]).reshape(-1, 8) if len(det) else np.zeros((0, 8))
    return np.trunc(ordered).astype(np.int64), ordered
