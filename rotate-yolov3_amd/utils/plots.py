"""Pictures with the boxes drawn in: plot_one_box and plot_images of the reference (utils/utils.py:479-490, :514-550) over
ryolo_det_corners and ryolo_draw_quads (csrc/detpost.hip, csrc/draw.hip).  The pixels stay on the device until they are encoded; the host
renders the label texts once each (Pillow's built-in font, cached) and hands them over as one-byte-per-pixel bitmaps.

The outline is the port's own exact integer definition (include/ryolo.h), not cv2.polylines'; the label is upright with its bottom left
at the box's corner 0, where cv2.putText puts its origin."""
import math
import os

import numpy as np
import torch

from ..model import hip_ops

DEFAULT_CLASSES = 80         # colours made when no class names are known (classes beyond the table wrap around)
_FONTS = {}
_LABELS = {}


def class_colors(nc, seed=0):
    """uint8 [nc, 3]: one RGB colour per class from np.random.default_rng(seed) (the reference draws them unseeded, detect.py:199)"""
    return np.random.default_rng(int(seed)).integers(0, 256, (max(int(nc), 0), 3), dtype=np.uint8)


def line_thickness(h, w):
    """plot_one_box's default: round(0.002 * (h + w) / 2) + 1"""
    return round(0.002 * (h + w) / 2) + 1


def load_class_names(data):
    """the lines of the `names` file of a *.data file (load_classes(parse_data_cfg(data)['names']) of the reference); None when either
    file is missing"""
    from .parse_config import parse_data_cfg
    if not (data and os.path.isfile(data)):
        return None
    path = parse_data_cfg(data).get('names', '')
    if not os.path.isfile(path):
        return None
    with open(path, 'r') as f:
        return [x for x in f.read().split('\n') if x]


def _font(size):
    if size not in _FONTS:
        try:
            from PIL import ImageFont
        except ImportError:
            raise RuntimeError("the labels are rendered with Pillow, which is not installed (pip install pillow)")
        try:
            _FONTS[size] = ImageFont.load_default(size=size)      # the font built into Pillow: no font file is looked for
        except TypeError:                                          # an older Pillow: its fixed-size bitmap font
            _FONTS[size] = ImageFont.load_default()
    return _FONTS[size]


def render_label(text, tl):
    """uint8 0/1 bitmap [lh, lw] of `text` in Pillow's built-in font at size max(10, 7 * tl) (tl: the line thickness), coverage
    thresholded at 128, cropped to the text's box.  Cached by (text, tl); the array is read-only."""
    key = (str(text), int(tl))
    if key not in _LABELS:
        from PIL import Image, ImageDraw
        font = _font(max(10, 7 * int(tl)))
        probe = ImageDraw.Draw(Image.new('L', (1, 1)))
        x0, y0, x1, y1 = probe.textbbox((0, 0), key[0], font=font)
        lw, lh = max(int(math.ceil(x1 - x0)), 1), max(int(math.ceil(y1 - y0)), 1)
        im = Image.new('L', (lw, lh), 0)
        ImageDraw.Draw(im).text((-x0, -y0), key[0], fill=255, font=font)
        bits = (np.asarray(im, dtype=np.uint8) >= 128).astype(np.uint8)
        bits.setflags(write=False)
        _LABELS[key] = bits
    return _LABELS[key]


def pack_labels(bitmaps, anchors):
    """(lab_bits, lab_off, lab_rect) of ryolo_draw_quads: the bitmaps ([lh, lw] uint8, None: no label) back to back, their byte offsets
    (int64 [M]) and their rectangles (int32 [M, 4] rows x, y, w, h) with the bottom left at the row's anchor (X0, Y0), the quad's corner 0:
    (X0, Y0 - lh, lw, lh).  anchors: integer [M, 2] -- a numpy array or a list gives numpy arrays, a torch tensor gives tensors on its
    device (the rectangles are then put together there: the anchors are never downloaded)."""
    m = len(bitmaps)
    sizes = np.zeros((m, 2), dtype=np.int64)             # lw, lh
    for k, bm in enumerate(bitmaps):
        if bm is not None and bm.size:
            if bm.ndim != 2 or bm.dtype != np.uint8:
                raise ValueError("a label bitmap is a uint8 [lh, lw] array, not %s %s" % (bm.dtype, bm.shape))
            sizes[k] = (bm.shape[1], bm.shape[0])
    nbytes = sizes[:, 0] * sizes[:, 1]
    off = np.concatenate(([0], np.cumsum(nbytes)[:-1])).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    parts = [np.ascontiguousarray(bm).reshape(-1) for bm, nb in zip(bitmaps, nbytes) if nb]
    bits = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    if torch.is_tensor(anchors):
        if anchors.is_floating_point() or tuple(anchors.shape) != (m, 2):
            raise ValueError("anchors must be integer [M, 2], not %s %s" % (anchors.dtype, tuple(anchors.shape)))
        dev = anchors.device
        wh = torch.from_numpy(sizes.astype(np.int32)).to(dev)
        a = anchors.to(torch.int32)
        rect = torch.stack((a[:, 0], a[:, 1] - wh[:, 1], wh[:, 0], wh[:, 1]), 1).contiguous()
        return torch.from_numpy(bits).to(dev), torch.from_numpy(off).to(dev), rect
    a = np.asarray(anchors).reshape(m, 2)
    if a.dtype.kind not in 'iu':
        raise ValueError("anchors must be integer [M, 2], not %s" % a.dtype)
    rect = np.stack((a[:, 0], a[:, 1] - sizes[:, 1], sizes[:, 0], sizes[:, 1]), 1).astype(np.int32)
    return bits, off, rect


def label_text(names, cls, conf):
    """'%s %.2f' % (names[int(cls)], conf) of the reference (detect.py:244); the class index where the class has no name"""
    c = int(cls)
    return '%s %.2f' % (names[c] if names is not None and 0 <= c < len(names) else c, conf)


def draw_detections(cache, n, det, det_off, names, colors, thick=None, host_rows=None):
    """plot_one_box for every detection of a batch: -> the drawn copy of the batch's pixels (uint8, laid out like cache.pixels, on the
    device); the cache itself stays as it was.
    cache: the device cache of the batch's n images; det: fp32 [M, 8] rows in the images' own pixels and det_off: int32 [n + 1], both on
    the device (utils.detect_images.detect_images); names: class names or None; colors: uint8 [nc, 3] (class_colors; classes beyond it
    wrap around); thick: None (line_thickness per image), one int, or one per image; host_rows: det as a list of rows where the caller
    has downloaded it already (otherwise det is downloaded here: the texts need the classes and the scores)."""
    if cache.n != n or det_off.numel() != n + 1:
        raise ValueError("draw_detections: %d images, a cache of %d, %d offsets" % (n, cache.n, det_off.numel()))
    dev = cache.pixels.device
    if thick is None:
        thick = [line_thickness(h, w) for h, w in cache.hw]
    thick = np.clip(np.broadcast_to(np.asarray(thick, dtype=np.int64), (n,)), 1, 255)
    quad = hip_ops.det_corners(det)
    m = det.shape[0]
    rows = det.cpu().tolist() if host_rows is None else host_rows
    off = det_off.cpu().tolist()
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    color = np.zeros((m, 4), dtype=np.uint8)
    bitmaps = []
    for b in range(n):
        for r in range(off[b], off[b + 1]):
            cls, conf = rows[r][7], rows[r][5]
            if len(colors):
                color[r, :3] = colors[int(cls) % len(colors)]
            bitmaps.append(render_label(label_text(names, cls, conf), int(thick[b])))
    labels = pack_labels(bitmaps, quad[:, :2]) if m else None
    return hip_ops.draw_quads(cache, quad, det_off, torch.from_numpy(color).to(dev), thick, labels=labels)


def mosaic_rows(targets, n, ns, h, w):
    """the targets (img, cls, cx, cy, w, h, a; normalised) of the first n images as fp32 [k, 8] rows in the pixels of an ns x ns mosaic
    of h x w cells, image i in cell (i // ns, i % ns), ordered by image (within an image: as they come) -- in float32, product then sum"""
    t = np.asarray(targets, dtype=np.float32).reshape(-1, 7)
    t = t[t[:, 0] < n]
    t = t[np.argsort(t[:, 0], kind='stable')]
    i = t[:, 0].astype(np.int64)
    det = np.zeros((len(t), 8), dtype=np.float32)
    det[:, 0] = t[:, 2] * np.float32(w) + ((i % ns) * w).astype(np.float32)
    det[:, 1] = t[:, 3] * np.float32(h) + ((i // ns) * h).astype(np.float32)
    det[:, 2] = t[:, 4] * np.float32(w)
    det[:, 3] = t[:, 5] * np.float32(h)
    det[:, 4] = t[:, 6]
    return det


def plot_images(batch, targets, fname, max_images=16, seed=0):
    """The reference's train_batch0.jpg: the first min(bs, max_images) images of an NHWC8Batch tiled into a ceil(sqrt(n)) x ceil(sqrt(n))
    mosaic at their own size (the pixels x 255 truncated to uint8; cells without an image are black), every target drawn as a rotated
    outline of thickness 2 in a random colour of its own (np.random.default_rng(seed)), saved with Pillow (JPEG at quality 95).  The
    mosaic is one image to ryolo_draw_quads, so each side is at most 16384.  Returns the drawn mosaic, uint8 [ns h, ns w, 3], on the device.
    Once per run: torch ops build the mosaic."""
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("plot_images saves with Pillow, which is not installed (pip install pillow)")
    data = batch.data
    dev = data.device
    bs, h, w, _ = data.shape
    n = min(bs, int(max_images))
    ns = int(math.ceil(n ** 0.5))
    mosaic = torch.zeros((ns * h, ns * w, 3), dtype=torch.uint8, device=dev)
    for i in range(n):
        cell = (data[i, :, :, :3].float() * 255.0).clamp_(0.0, 255.0).to(torch.uint8)
        mosaic[(i // ns) * h:(i // ns + 1) * h, (i % ns) * w:(i % ns + 1) * w] = cell
    det = mosaic_rows(targets.detach().cpu().numpy() if torch.is_tensor(targets) else targets, n, ns, h, w)
    color = np.zeros((len(det), 4), dtype=np.uint8)
    color[:, :3] = np.random.default_rng(int(seed)).integers(0, 256, (len(det), 3), dtype=np.uint8)
    quad = hip_ops.det_corners(torch.from_numpy(det).to(dev))
    pixels = (mosaic.reshape(-1), torch.zeros(1, dtype=torch.int64, device=dev),
              torch.tensor([[ns * h, ns * w]], dtype=torch.int32, device=dev), [(ns * h, ns * w)])
    det_off = torch.tensor([0, len(det)], dtype=torch.int32, device=dev)
    hip_ops.draw_quads(pixels, quad, det_off, torch.from_numpy(color).to(dev), 2, out=pixels[0])
    save_image(mosaic.cpu().numpy(), fname)
    return mosaic


def save_image(array, path):
    """an RGB uint8 [h, w, 3] array to `path` as its extension says: PNG stays PNG, JPEG at quality 95, the others as Pillow writes them"""
    from PIL import Image
    kw = {'quality': 95} if os.path.splitext(path)[-1].lower() in ('.jpg', '.jpeg') else {}
    Image.fromarray(array).save(path, **kw)
