"""The real-data input path: image list -> device image cache -> one ryolo_letterbox_augment launch per batch (csrc/augment.hip) -> NHWC8Batch,
with the labels transformed on the host by the reference's arithmetic (utils/datasets.py LoadImagesAndLabels / letterbox,
utils/augment.py Transform / random_affine, utils/utils.py get_rotated_coors -- restated here, not imported: no OpenCV, no imgaug).

Two coordinate conventions meet here, as they do in the reference.  Labels live in continuous pixel coordinates (cx * w): their maps are
`*.label` / label_matrix().  Pixels are addressed by index, and cv2.warpAffine applies the SAME matrix to indices, so the picture and its
labels differ by the half-pixel terms of scale and rotation (below 0.6 px at the reference's ranges); image_matrix() keeps that.  The
flips are exact on both sides: index x -> W - 1 - x (np.fliplr), label x -> W - x.  DESIGN.md section 3.10 lists every deviation from
OpenCV / imgaug (bilinear sampling, one pass, no uint8 rounding between stages, the closed-form saturation / value stage, the noise)."""
import collections
import math
import os

import numpy as np
import torch

NPARAM = 16              # == ryolo_aug_nparam()
MAX_BLUR_SIGMA = 1.5     # == ryolo_aug_max_blur_sigma(): the kernel's 9-tap window holds +-2.67 sigma of it
IMG_FORMATS = ('.bmp', '.jpg', '.jpeg', '.png', '.tif', '.dng')
# Transform([...]) of the reference's __getitem__ (datasets.py:471-482): the probability of each stage
PROBS = dict(affine=0.5, noise=0.2, gamma=0.4, blur=0.5, hsv=0.5, hflip=0.5, vflip=0.5, gray=0.5)

Letterbox = collections.namedtuple('Letterbox', 'ratio new_unpad dw dh top left image label')
# affine: None or (a_deg, s, tx_unit, ty_unit) -- the translations in units of the image side, as drawn
AugDraw = collections.namedtuple('AugDraw', 'affine noise_sigma gamma blur_sigma sat_gain val_gain hflip vflip gray_alpha')
NEUTRAL = AugDraw(None, 0.0, 1.0, 0.0, 1.0, 1.0, False, False, 0.0)


def letterbox_matrix(h, w, new_shape):
    """letterbox(img, new_shape, mode='square') of an h x w image as two 3x3 maps from source to output coordinates:
    .label, what the reference applies to the labels (ratio * x + dw: the unrounded half paddings), and .image, where the pixels go
    (resize to new_unpad with aligned pixel centres, then the rounded top / left padding)."""
    ratio = float(new_shape) / max(h, w)
    new_unpad = (int(round(w * ratio)), int(round(h * ratio)))       # (width, height)
    dw = (new_shape - new_unpad[0]) / 2
    dh = (new_shape - new_unpad[1]) / 2
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    sx, sy = new_unpad[0] / w, new_unpad[1] / h
    image = np.array([[sx, 0.0, 0.5 * sx - 0.5 + left], [0.0, sy, 0.5 * sy - 0.5 + top], [0.0, 0.0, 1.0]])
    label = np.array([[ratio, 0.0, dw], [0.0, ratio, dh], [0.0, 0.0, 1.0]])
    return Letterbox(ratio, new_unpad, dw, dh, top, left, image, label)


def affine_matrix(a_deg, s, tx, ty, W, H):
    """M = T @ R of random_affine: R = cv2.getRotationMatrix2D(angle=a_deg, center=(W / 2, H / 2), scale=s), T the translation (tx, ty)"""
    a = math.radians(a_deg)
    alpha, beta = s * math.cos(a), s * math.sin(a)
    cx, cy = W / 2, H / 2
    R = np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy], [0.0, 0.0, 1.0]])
    T = np.eye(3)
    T[0, 2], T[1, 2] = tx, ty
    return T @ R


def _affine_of(draw, size):
    a, s, tu, tv = draw.affine
    return affine_matrix(a, s, tu * size, tv * size, size, size)     # T[0, 2] = u * shape[0], T[1, 2] = v * shape[1]: a square


def label_matrix(draw, h, w, img_size):
    """source pixel coordinates (cx * w, cy * h) -> output pixel coordinates, as the reference moves the box centres"""
    M = letterbox_matrix(h, w, img_size).label
    if draw.affine is not None:
        M = _affine_of(draw, img_size) @ M
    if draw.hflip:
        M = np.array([[-1.0, 0.0, img_size], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ M
    if draw.vflip:
        M = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, img_size], [0.0, 0.0, 1.0]]) @ M
    return M


def image_matrix(draw, h, w, img_size):
    """source pixel index -> output pixel index: the forward map whose float64 inverse goes into the parameter row"""
    M = letterbox_matrix(h, w, img_size).image
    if draw.affine is not None:
        M = _affine_of(draw, img_size) @ M
    if draw.hflip:
        M = np.array([[-1.0, 0.0, img_size - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ M
    if draw.vflip:
        M = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, img_size - 1.0], [0.0, 0.0, 1.0]]) @ M
    return M


def param_row(draw, h, w, img_size, img_max=255.0):
    """the fp32 [16] parameter row of ryolo_letterbox_augment for one image: the inverse of image_matrix (float64, stored fp32), then
    noise_sigma, gamma, gamma_max (the cached image's maximum), blur_sigma, sat_gain, val_gain, gray_alpha, three zeros"""
    inv = np.linalg.inv(image_matrix(draw, h, w, img_size))
    row = np.zeros(NPARAM, dtype=np.float32)
    row[0:3], row[3:6] = inv[0], inv[1]
    row[6:13] = (draw.noise_sigma, draw.gamma, img_max, draw.blur_sigma, draw.sat_gain, draw.val_gain, draw.gray_alpha)
    return row


def draw_rng(seed, epoch, index):
    """the Generator of image `index` in epoch `epoch`: a batch does not depend on the iteration order or on the number of ranks"""
    return np.random.default_rng([int(seed), int(epoch), int(index)])


def draw_params(hyp, rng, probs=None):
    """One image's augmentation, drawn like Transform([...]) of the reference (datasets.py:471-482, utils/augment.py): each stage with its
    probability, its value from the hyp range.  hyp keys: degrees, translate, scale, noise, gamma, blur, hsv_s, hsv_v, grayscale (a missing
    one is 0; `shear` is ignored, as random_affine ignores it)."""
    p = dict(PROBS, **(probs or {}))
    g = lambda k: float(hyp.get(k, 0.0))      # noqa: E731
    if g('blur') > MAX_BLUR_SIGMA:
        raise ValueError("hyp['blur'] = %g exceeds the kernel's largest Gaussian sigma, %g" % (g('blur'), MAX_BLUR_SIGMA))
    affine, noise, gamma, blur, sat, val, alpha = None, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0
    if rng.random() < p['affine']:
        affine = (rng.uniform(-g('degrees'), g('degrees')), rng.uniform(1 - g('scale'), 1 + g('scale')),
                  rng.uniform(-g('translate'), g('translate')), rng.uniform(-g('translate'), g('translate')))
    if rng.random() < p['noise']:
        noise = rng.uniform(0.0, g('noise') * 255)                  # iaa.AdditiveGaussianNoise(scale=(0, intensity * 255))
    if rng.random() < p['gamma']:
        gamma = rng.uniform(1 - g('gamma'), 1 + g('gamma'))
    if rng.random() < p['blur']:
        blur = rng.uniform(0.0, g('blur'))                          # iaa.GaussianBlur(sigma=(0, sigma))
    if rng.random() < p['hsv']:
        sat = rng.uniform(-1, 1) * g('hsv_s') + 1
        val = rng.uniform(-1, 1) * g('hsv_v') + 1
    hflip = bool(rng.random() < p['hflip'])
    vflip = bool(rng.random() < p['vflip'])
    alpha0 = rng.uniform(g('grayscale'), 1.0)                       # Grayscale.__init__ draws its lower bound
    if rng.random() < p['gray']:
        alpha = rng.uniform(alpha0, 1.0)                            # iaa.Grayscale(alpha=(alpha0, 1.0))
    return AugDraw(affine, float(noise), float(gamma), float(blur), float(sat), float(val), hflip, vflip, float(alpha))


def wrap_angle(a):
    """random_affine's wrap of the box angle back towards (-pi/2, pi/2]: one step of pi, strict comparisons"""
    a = np.array(a, copy=True)
    a[a > 0.5 * math.pi] -= math.pi
    a[a < -0.5 * math.pi] += math.pi
    return a


def rotated_corners(boxes):
    """get_rotated_coors: [k, 5] (cx, cy, w, h, a) -> [k, 8] (x0, y0, .. x3, y3), the corners (xmin, ymin), (xmin, ymax), (xmax, ymax),
    (xmax, ymin) of the upright box turned by cv2.getRotationMatrix2D(angle=-a, center=(cx, cy), scale=1)"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    cx, cy, w, h, a = b.T
    alpha, beta = np.cos(-a), np.sin(-a)
    r02, r12 = (1 - alpha) * cx - beta * cy, beta * cx + (1 - alpha) * cy
    out = np.empty((len(b), 8))
    for k, (tx, ty) in enumerate(((cx - w * 0.5, cy - h * 0.5), (cx - w * 0.5, cy + h * 0.5), (cx + w * 0.5, cy + h * 0.5),
                                  (cx + w * 0.5, cy - h * 0.5))):
        out[:, 2 * k] = tx * alpha + ty * beta + r02
        out[:, 2 * k + 1] = tx * -beta + ty * alpha + r12
    return out


def keep_mask(t, width, height):
    """random_affine's filter on pixel-unit rows (cls, cx, cy, w, h, a): w > 4, h > 4, aspect ratio < 15 and all four corners strictly
    inside the image"""
    t = np.asarray(t)
    w, h = t[:, 3], t[:, 4]
    ar = np.maximum(w / (h + 1e-16), h / (w + 1e-16))
    c = rotated_corners(t[:, 1:6])
    xs, ys = c[:, 0::2], c[:, 1::2]
    return (w > 4) & (h > 4) & (ar < 15) & ((xs < width) & (xs > 0)).all(1) & ((ys < height) & (ys > 0)).all(1)


def transform_labels(labels, h, w, img_size, draw=NEUTRAL):
    """The label side of __getitem__ for one h x w (cached) image: normalised rows (cls, cx, cy, w, h, a) -> the normalised rows of the
    letterboxed, augmented img_size x img_size picture.  The reference's steps in its order, in the dtype of `labels`: letterbox ratio and
    offsets (datasets.py:463-467); under an affine draw the angle update and wrap, the centre through M, sizes * s, the clip and the
    filter (utils/augment.py:289-312); the flips (x -> W - x, a -> -a); the normalisation (datasets.py:488-490)."""
    t = np.array(labels, copy=True)
    if t.size == 0:
        return t.reshape(0, 6)
    lb = letterbox_matrix(h, w, img_size)
    t[:, 1] = lb.ratio * w * t[:, 1] + lb.dw
    t[:, 2] = lb.ratio * h * t[:, 2] + lb.dh
    t[:, 3] = lb.ratio * w * t[:, 3]
    t[:, 4] = lb.ratio * h * t[:, 4]
    if draw.affine is not None:
        a_deg, s = draw.affine[0], draw.affine[1]
        M = _affine_of(draw, img_size)
        t[:, 5] -= a_deg / 180 * math.pi
        t[:, 5] = wrap_angle(t[:, 5])
        cx = t[:, 1] * M[0, 0] + t[:, 2] * M[0, 1] + M[0, 2]
        cy = t[:, 1] * M[1, 0] + t[:, 2] * M[1, 1] + M[1, 2]
        t[:, 1], t[:, 2] = cx, cy
        t[:, [3, 4]] *= s
        t[:, 1] = t[:, 1].clip(0, img_size)
        t[:, 2] = t[:, 2].clip(0, img_size)
        t = t[keep_mask(t, img_size, img_size)]
    if draw.hflip:
        t[:, 1] = img_size - t[:, 1]
        t[:, 5] = -t[:, 5]
    if draw.vflip:
        t[:, 2] = img_size - t[:, 2]
        t[:, 5] = -t[:, 5]
    t[:, [2, 4]] /= img_size
    t[:, [1, 3]] /= img_size
    return t


def label_path_of(img_path):
    """the reference's rule (datasets.py:283): 'images' -> 'labels', the extension -> '.txt'"""
    return img_path.replace('images', 'labels').replace(os.path.splitext(img_path)[-1], '.txt')


def check_labels(l, file='labels'):
    """the four assertions of the reference's label reader (datasets.py:340-343) on a [k, 6] array"""
    if l.shape[0]:
        if l.ndim != 2 or l.shape[1] != 6:
            raise ValueError('> 6 label columns: %s' % file)
        if not (l[:, 1:-1] >= 0).all():
            raise ValueError('negative labels: %s' % file)
        if not (l[:, 1:-1] <= 1).all():
            raise ValueError('non-normalized or out of bounds coordinate labels: %s' % file)
        if not ((l[:, 5] < math.pi / 2).all() and (l[:, 5] > -math.pi / 2).all()):
            raise ValueError('out of angle bounds (-0.5pi,0.5pi): %s' % file)
    return l


def read_labels(path):
    """[k, 6] float32 rows (cls, cx, cy, w, h, a) of a label file; a missing or empty file is no labels"""
    if not os.path.isfile(path):
        return np.zeros((0, 6), dtype=np.float32)
    with open(path, 'r') as f:
        rows = [x.split() for x in f.read().splitlines() if x.strip()]
    if not rows:
        return np.zeros((0, 6), dtype=np.float32)
    if len(set(len(r) for r in rows)) != 1:
        raise ValueError('> 6 label columns: %s' % path)
    return check_labels(np.array(rows, dtype=np.float32), path)


class DeviceImageCache(object):
    """Every image of a list decoded once and kept on the GPU as RGB uint8 HWC, back to back: .pixels, .img_offset (int64 [n], bytes),
    .img_hw (int32 [n, 2]); on the host .hw (cached sizes), .shapes (sizes on disk) and .maxima (largest byte per image, gamma's scale).
    An image whose long side exceeds img_size is reduced once with Image.BOX to letterbox's new_unpad, so the kernel never minifies.
    The whole set must fit in cache_limit_bytes: there is no streaming from disk."""

    def __init__(self, paths, img_size, device, cache_limit_bytes=8 << 30):
        try:
            from PIL import Image
        except ImportError:
            raise RuntimeError("DeviceImageCache decodes images with Pillow, which is not installed (pip install pillow)")
        arrays, shapes, total = [], [], 0
        for path in paths:
            with Image.open(path) as im:
                im = im.convert('RGB')
                w0, h0 = im.size
                if max(h0, w0) > img_size:
                    im = im.resize(letterbox_matrix(h0, w0, img_size).new_unpad, Image.BOX)
                a = np.asarray(im, dtype=np.uint8)
            total += a.nbytes
            if total > cache_limit_bytes:
                raise RuntimeError("image cache: %d images need more than cache_limit_bytes = %d (at %s); streaming from disk is not "
                                   "implemented" % (len(paths), cache_limit_bytes, path))
            arrays.append(a)
            shapes.append((h0, w0))
        self._upload(arrays, shapes, device)

    @classmethod
    def from_arrays(cls, arrays, device):
        """a cache of in-memory RGB uint8 [h, w, 3] arrays, taken as they are"""
        self = cls.__new__(cls)
        arrays = [np.ascontiguousarray(a, dtype=np.uint8) for a in arrays]
        for a in arrays:
            if a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise ValueError("an image is an RGB uint8 [h, w, 3] array, not %s" % (a.shape,))
        self._upload(arrays, [a.shape[:2] for a in arrays], device)
        return self

    def _upload(self, arrays, shapes, device):
        if not arrays:
            raise ValueError("image cache: no images")
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("the image cache lives on a GPU: ryolo_letterbox_augment has no CPU path")
        sizes = [a.nbytes for a in arrays]
        offsets = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
        self.n = len(arrays)
        self.nbytes = int(sum(sizes))
        self.hw = [tuple(int(v) for v in a.shape[:2]) for a in arrays]
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.maxima = np.array([a.max() for a in arrays], dtype=np.float32)
        self.pixels = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(device)
        self.img_offset = torch.from_numpy(offsets).to(device)
        self.img_hw = torch.tensor(self.hw, dtype=torch.int32).reshape(self.n, 2).to(device)


class LoadImagesAndLabels(object):
    """The reference's training / evaluation loader on the device path.  `path`: a list file of image paths; labels by label_path_of.
    Yields (NHWC8Batch [bs, 3, S, S], targets [nt, 7] (img, cls, cx, cy, w, h, a) on the device, paths, shapes) like collate_fn.
    augment=True draws every image's augmentation from (seed, epoch, image index) and shuffles the epoch by (seed, epoch); this rank
    serves the images order[rank::world].  set_epoch(e) selects the epoch."""

    def __init__(self, path, img_size=416, batch_size=16, augment=False, hyp=None, rect=False, image_weights=False, rank=0, world=1,
                 seed=0, device='cuda', cache_limit_bytes=8 << 30):
        if rect or image_weights:
            raise NotImplementedError("rect=True / image_weights=True: the device loader serves square letterboxed batches in list order "
                                      "or shuffled")
        with open(str(path), 'r') as f:
            self.img_files = [x.replace('/', os.sep) for x in f.read().splitlines() if os.path.splitext(x)[-1].lower() in IMG_FORMATS]
        if not self.img_files:
            raise ValueError('No images found in %s' % path)
        if not (0 <= rank < world):
            raise ValueError('rank %d of %d' % (rank, world))
        self.label_files = [label_path_of(x) for x in self.img_files]
        self.labels = [read_labels(x) for x in self.label_files]
        self.n = len(self.img_files)
        self.img_size, self.batch_size, self.augment, self.hyp = int(img_size), int(batch_size), bool(augment), hyp or {}
        self.rank, self.world, self.seed, self.epoch = int(rank), int(world), int(seed), 0
        self.device = torch.device(device)
        self.cache = DeviceImageCache(self.img_files, self.img_size, self.device, cache_limit_bytes)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        """the image indices this rank serves in the current epoch, in order"""
        order = np.random.default_rng([self.seed, self.epoch]).permutation(self.n) if self.augment else np.arange(self.n)
        return order[self.rank::self.world]

    def __len__(self):
        return (len(range(self.rank, self.n, self.world)) + self.batch_size - 1) // self.batch_size

    def draw(self, index):
        return draw_params(self.hyp, draw_rng(self.seed, self.epoch, index)) if self.augment else NEUTRAL

    def __iter__(self):
        from ..model import hip_ops
        idx = self.indices()
        S = self.img_size
        for b in range(0, len(idx), self.batch_size):
            chunk = [int(i) for i in idx[b:b + self.batch_size]]
            rows, targets = np.empty((len(chunk), NPARAM), dtype=np.float32), []
            for slot, i in enumerate(chunk):
                h, w = self.cache.hw[i]
                d = self.draw(i)
                rows[slot] = param_row(d, h, w, S, self.cache.maxima[i])
                t = transform_labels(self.labels[i], h, w, S, d)
                targets.append(np.concatenate((np.full((len(t), 1), slot, dtype=np.float32), t.astype(np.float32)), 1))
            # the noise field of a batch: keyed by its first image, so it too is independent of the iteration history
            noise_seed = int(np.random.SeedSequence([self.seed, self.epoch, chunk[0], 1]).generate_state(1, np.uint64)[0] >> np.uint64(1))
            batch = hip_ops.letterbox_augment(self.cache, torch.tensor(chunk, dtype=torch.int32).to(self.device),
                                              torch.from_numpy(rows).to(self.device), noise_seed, S, S)
            yield (batch, torch.from_numpy(np.concatenate(targets, 0)).to(self.device), tuple(self.img_files[i] for i in chunk),
                   tuple(self.cache.shapes[i] for i in chunk))


VID_FORMATS = ('.mov', '.avi', '.mp4', '.mpg', '.mpeg', '.m4v', '.wmv', '.mkv')


def place_rows(shapes, size):
    """the int32 [N, 4] rows (left, top, new_w, new_h) of ryolo_letterbox_area: where letterbox_matrix puts each (h, w) image of `shapes`
    in a size x size batch.  A side that would round to 0 pixels is 1 (cv2.resize of the reference fails there)."""
    rows = np.empty((len(shapes), 4), dtype=np.int32)
    for k, (h, w) in enumerate(shapes):
        lb = letterbox_matrix(h, w, size)
        new_w, new_h = max(lb.new_unpad[0], 1), max(lb.new_unpad[1], 1)
        rows[k] = (min(lb.left, size - new_w), min(lb.top, size - new_h), new_w, new_h)
    return rows


def is_video_or_stream(path):
    """a camera number, a stream URL or a path with a video extension: what the reference hands to cv2.VideoCapture"""
    path = str(path)
    return (path.isdigit() or path.startswith(('rtsp://', 'rtmp://', 'http://', 'https://'))
            or os.path.splitext(path)[-1].lower() in VID_FORMATS)


def list_images(path):
    """the image files `path` names: a directory (sorted, filtered by IMG_FORMATS), one image file, or a .txt list of paths"""
    path = str(path)
    ext = os.path.splitext(path)[-1].lower()
    if is_video_or_stream(path):
        raise NotImplementedError("LoadImages: %r is a video or a stream; this port decodes still images with Pillow and has no OpenCV "
                                  "(extract the frames to a directory of images)" % path)
    if os.path.isdir(path):
        names = sorted(os.listdir(path))
        videos = [x for x in names if os.path.splitext(x)[-1].lower() in VID_FORMATS]
        if videos:
            raise NotImplementedError("LoadImages: %s holds video files (%s ...); this port decodes still images with Pillow and has no "
                                      "OpenCV" % (path, videos[0]))
        files = [os.path.join(path, x) for x in names if os.path.splitext(x)[-1].lower() in IMG_FORMATS]
    elif ext == '.txt' and os.path.isfile(path):
        with open(path, 'r') as f:
            files = [x.strip().replace('/', os.sep) for x in f.read().splitlines()]
        files = [x for x in files if os.path.splitext(x)[-1].lower() in IMG_FORMATS]
    elif ext in IMG_FORMATS and os.path.isfile(path):
        files = [path]
    else:
        raise FileNotFoundError("LoadImages: %r is neither a directory, an image file %s nor a .txt list" % (path, IMG_FORMATS))
    if not files:
        raise ValueError('No images found in %s' % path)
    return files


class LoadImages(object):
    """The reference's inference loader (utils/datasets.py LoadImages) on the device path.  Per batch of batch_size files Pillow decodes to
    RGB and the ORIGINAL pixels are uploaded once (DeviceImageCache.from_arrays): nothing is resized on the host, ryolo_letterbox_area
    writes the batch at whatever size is asked for.  Yields (paths, cache, shapes): the files of the batch, their device cache, their
    (h, w).  letterbox_batch(cache, shapes, size, slots=batch_size) makes the NHWC8Batch: always batch_size slots, so one engine shape
    serves the whole run; the slots past the images (the last batch) have src_index -1, are all border, and their results are dropped.
    img_size is the reference's argument and is only kept (.img_size): the loader resizes nothing, the size is letterbox_batch's."""

    def __init__(self, path, img_size=416, batch_size=8, device='cuda'):
        self.files = list_images(path)
        self.img_size, self.batch_size, self.device = int(img_size), int(batch_size), torch.device(device)
        if self.batch_size < 1:
            raise ValueError('batch_size %d' % self.batch_size)

    def __len__(self):
        return (len(self.files) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        try:
            from PIL import Image
        except ImportError:
            raise RuntimeError("LoadImages decodes images with Pillow, which is not installed (pip install pillow)")
        for b in range(0, len(self.files), self.batch_size):
            paths = tuple(self.files[b:b + self.batch_size])
            arrays = []
            for p in paths:
                with Image.open(p) as im:
                    arrays.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
            cache = DeviceImageCache.from_arrays(arrays, self.device)
            yield paths, cache, tuple(cache.hw)


def letterbox_batch(cache, shapes, size, slots=None, out=None):
    """ryolo_letterbox_area of the len(shapes) images of `cache` into `slots` >= len(shapes) slots of size x size; the slots past the
    images read nothing (src_index -1)"""
    from ..model import hip_ops
    n = len(shapes)
    slots = n if slots is None else int(slots)
    if slots < n:
        raise ValueError('%d images do not fit %d slots' % (n, slots))
    src = torch.tensor(list(range(n)) + [-1] * (slots - n), dtype=torch.int32).to(cache.pixels.device)
    place = np.concatenate((place_rows(shapes, size), np.tile(np.array([[0, 0, 1, 1]], dtype=np.int32), (slots - n, 1))), 0)
    return hip_ops.letterbox_area(cache, src, place, size, size, out)
