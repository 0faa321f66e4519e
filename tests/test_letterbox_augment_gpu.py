"""GPU tier: ryolo_letterbox_augment (csrc/augment.hip) against the float64 oracle tests/augment_reference.py.

The rule of every comparison: an output o (bf16) must be the round-to-nearest-even bf16 of SOME value in [v - eps, v + eps], v the
oracle's float64 value in [0, 1] units -- checked exactly, by intersecting that interval with the set of reals that round to o.  No
pixel is excluded.  eps:
  geometry only   6 * max(H, W) * 2^-24: three fp32 roundings of a coordinate of magnitude max(H, W) (half an ulp each, on either axis)
                  times the largest pixel-to-pixel step, 1.0.  Derived, not tuned.
  photometric     measured on the test's own inputs: 8 x the largest difference between the oracle evaluated in float32 and in float64
                  (the margin is for device powf / logf / cosf being a few ulp off numpy's), never below the geometric eps.  Printed.
Every output buffer is pre-filled with NaN bits, so an element the kernel does not write fails the comparison."""
import math

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model.nhwc_batch import NHWC8Batch
from rotate_yolov3_amd.utils import datasets as ds
from tests import augment_reference as ref

pytestmark = pytest.mark.gpu

_rng = np.random.default_rng(2016)
IMAGES = [_rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((37, 53), (64, 64), (1, 1), (90, 30))]
SRC = [2, 0, 0, 3]
SHAPES = [(64, 64), (40, 72)]          # (H, W): whole tiles; partial tiles on both axes
NEUTRAL = dict(noise=0.0, gamma=1.0, gamma_max=255.0, blur=0.0, sat=1.0, val=1.0, alpha=0.0)


def geo_eps(H, W):
    return 6 * max(H, W) * 2.0 ** -24


def row_of(F, **photo):
    """parameter row from a FORWARD map (source pixel index -> output pixel index): inverted in float64, stored fp32"""
    p = dict(NEUTRAL, **photo)
    inv = np.linalg.inv(F)
    return np.array(list(inv[0]) + list(inv[1]) + [p['noise'], p['gamma'], p['gamma_max'], p['blur'], p['sat'], p['val'], p['alpha'], 0, 0, 0],
                    dtype=np.float32)


def fit(h, w, H, W):
    """letterbox of an h x w source into H x W: one ratio, centred, pixel centres aligned"""
    r = min(H / h, W / w)
    return np.array([[r, 0, 0.5 * r - 0.5 + (W - w * r) / 2], [0, r, 0.5 * r - 0.5 + (H - h * r) / 2], [0, 0, 1.0]])


def flip(H, W, hor, ver):
    return np.array([[-1.0 if hor else 1.0, 0, W - 1.0 if hor else 0.0], [0, -1.0 if ver else 1.0, H - 1.0 if ver else 0.0], [0, 0, 1.0]])


GEOMETRY = {
    "letterbox": lambda h, w, H, W: fit(h, w, H, W),
    "rot5": lambda h, w, H, W: ds.affine_matrix(5.0, 1.0, 0, 0, W, H) @ fit(h, w, H, W),
    "scale085": lambda h, w, H, W: ds.affine_matrix(0.0, 0.85, 0, 0, W, H) @ fit(h, w, H, W),
    "scale115": lambda h, w, H, W: ds.affine_matrix(0.0, 1.15, 0, 0, W, H) @ fit(h, w, H, W),
    "translate": lambda h, w, H, W: ds.affine_matrix(0.0, 1.0, 3.3, -2.7, W, H) @ fit(h, w, H, W),
    "flips": lambda h, w, H, W: flip(H, W, True, True) @ fit(h, w, H, W),
    "all": lambda h, w, H, W: flip(H, W, True, False) @ ds.affine_matrix(-5.0, 1.15, -2.2, 4.1, W, H) @ fit(h, w, H, W),
}


def rows_for(images, src, H, W, geometry="letterbox", **photo):
    return np.stack([row_of(GEOMETRY[geometry](images[s].shape[0], images[s].shape[1], H, W),
                            **dict(photo, gamma_max=float(images[s].max()) if 'gamma' in photo else 255.0)) for s in src])


@pytest.fixture(scope="module")
def cache(cuda_dev):
    return ds.DeviceImageCache.from_arrays(IMAGES, cuda_dev)


def poisoned(n, H, W, dev):
    return torch.full((n, H, W, 8), 0x7FC0, dtype=torch.int16, device=dev).view(torch.bfloat16)


def launch(cache, src, rows, seed, H, W, dev):
    """-> the output's bf16 bit patterns, uint32 [N, H, W, 8] on the host"""
    out = poisoned(len(src), H, W, dev)
    batch = ops.letterbox_augment(cache, torch.tensor(src, dtype=torch.int32, device=dev), torch.from_numpy(rows).to(dev), seed, H, W, out=out)
    assert isinstance(batch, NHWC8Batch) and batch.data.data_ptr() == out.data_ptr() and tuple(batch.shape) == (len(src), 3, H, W)
    torch.cuda.synchronize(dev)
    return out.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def _f64(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def assert_consistent(bits, v, eps, what):
    """every o is the nearest-even bf16 of some value in [v - eps, v + eps]; channels 3..7 are zero bits; nothing is NaN"""
    assert bits.shape[:3] == v.shape[:3] and bits.shape[3] == 8
    assert not bits[..., 3:].any(), "%s: channels 3..7 must be zero bits" % what
    o = bits[..., :3]
    assert (o <= 0x3F80).all(), "%s: %d values are NaN, negative or above 1" % (what, int((o > 0x3F80).sum()))
    prev = np.where(o == 0, 0x8001, o - 1)
    lo_mid, hi_mid = (_f64(prev) + _f64(o)) / 2, (_f64(o) + _f64(o + 1)) / 2
    even = (o & 1) == 0                      # a tie rounds to the even neighbour: the cell of an even o is closed
    ok_lo = np.where(even, v + eps >= lo_mid, v + eps > lo_mid)
    ok_hi = np.where(even, v - eps <= hi_mid, v - eps < hi_mid)
    bad = ~(ok_lo & ok_hi)
    err = np.abs(_f64(o) - v)
    print("%s: eps %.3g, largest |o - v| %.3g (bf16 spacing near 1: %.3g), %d of %d outside" % (what, eps, err.max(), 2.0 ** -8, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: worst %s" % (what, [(tuple(i), hex(int(o[tuple(i)])), float(v[tuple(i)])) for i in np.argwhere(bad)[:5]])


def measured_eps(images, src, rows, seed, H, W):
    v64 = ref.augment(images, src, rows, seed, H, W, np.float64)
    v32 = ref.augment(images, src, rows, seed, H, W, np.float32)
    m = float(np.abs(v32.astype(np.float64) - v64).max())
    return v64, max(8 * m, geo_eps(H, W)), m


# ------------------------------------------------------------------------------------------------ identity, flips, integer shifts
@pytest.mark.parametrize("name,F", [
    ("identity", np.eye(3)),
    ("hflip", flip(64, 64, True, False)), ("vflip", flip(64, 64, False, True)), ("both", flip(64, 64, True, True)),
    ("shift", np.array([[1.0, 0, 5], [0, 1.0, -7], [0, 0, 1]])),
])
def test_pure_index_maps_equal_the_fp32_converter_bit_for_bit(cuda_dev, cache, name, F):
    """the new producer makes what ryolo_nchw_f32_to_nhwc_bf16 makes of u8 / 255 -- the batch the engines have accepted so far"""
    img = IMAGES[1]
    want_u8 = np.full((64, 64, 3), 128, dtype=np.uint8)
    for y in range(64):
        for x in range(64):
            sx, sy = np.linalg.inv(F)[:2] @ np.array([x, y, 1.0])
            sx, sy = int(round(sx)), int(round(sy))
            if 0 <= sx < 64 and 0 <= sy < 64:
                want_u8[y, x] = img[sy, sx]
    x32 = torch.from_numpy(want_u8.astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None].contiguous().to(cuda_dev)
    want = ops.nchw_f32_to_nhwc_bf16(x32)
    bits = launch(cache, [1], row_of(F)[None], 0, 64, 64, cuda_dev)
    assert np.array_equal(bits, want.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF)
    assert not bits[..., 3:].any()


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_geometry_only(cuda_dev, cache, geometry, H, W):
    rows = rows_for(IMAGES, SRC, H, W, geometry)
    v = ref.augment(IMAGES, SRC, rows, 0, H, W)
    assert_consistent(launch(cache, SRC, rows, 0, H, W, cuda_dev), v, geo_eps(H, W), "%s %dx%d" % (geometry, H, W))


# ------------------------------------------------------------------------------------------------ photometric stages
def _colour_image():
    """grey, black, white, fully saturated and random pixels, in blocks and singly"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)
    a[:12, :12] = rng.integers(0, 256, (12, 12, 1), dtype=np.uint8)      # greys, each its own level
    a[:12, 12:24] = 0
    a[12:24, :12] = 255
    a[12:24, 12:24] = (255, 0, 0)
    a[24:36, :12] = (0, 255, 255)
    a[24:36, 12:24] = (1, 0, 0)
    a[36:, :12][::2, ::2] = 0
    return a


PHOTO_IMAGES = [_colour_image(), IMAGES[0], IMAGES[3], np.zeros((64, 64, 3), dtype=np.uint8)]
PHOTO_SRC = [0, 1, 2, 0]
PHOTO = {
    "noise": dict(noise=2.55),
    "gamma08": dict(gamma=0.8), "gamma12": dict(gamma=1.2),
    "blur04": dict(blur=0.4), "blur15": dict(blur=1.5), "blur_above_the_limit": dict(blur=4.0),
    "gains_sat05_val15": dict(sat=0.5, val=1.5), "gains_sat15_val05": dict(sat=1.5, val=0.5), "gains_both15": dict(sat=1.5, val=1.5),
    "gray03": dict(alpha=0.3), "gray1": dict(alpha=1.0),
    "together": dict(noise=2.55, gamma=0.8, blur=1.5, sat=1.5, val=0.5, alpha=0.3),
    "together2": dict(noise=2.55, gamma=1.2, blur=0.4, sat=0.5, val=1.5, alpha=1.0),
}


@pytest.fixture(scope="module")
def photo_cache(cuda_dev):
    return ds.DeviceImageCache.from_arrays(PHOTO_IMAGES, cuda_dev)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("stage", sorted(PHOTO))
def test_photometric_stages(cuda_dev, photo_cache, stage, H, W):
    # slots 0..2 through the combined geometry, slot 3 the colour image through the plain letterbox
    rows = rows_for(PHOTO_IMAGES, PHOTO_SRC, H, W, "all", **PHOTO[stage])
    rows[3] = rows_for(PHOTO_IMAGES, PHOTO_SRC, H, W, "letterbox", **PHOTO[stage])[3]
    v, eps, m = measured_eps(PHOTO_IMAGES, PHOTO_SRC, rows, 77, H, W)
    print("%s %dx%d: oracle float32 vs float64 differ by at most %.3g -> eps %.3g (geometric floor %.3g)" % (stage, H, W, m, eps, geo_eps(H, W)))
    assert_consistent(launch(photo_cache, PHOTO_SRC, rows, 77, H, W, cuda_dev), v, eps, "%s %dx%d" % (stage, H, W))


# ------------------------------------------------------------------------------------------------ blur: seams and edges
def test_blur_of_single_pixels_across_tile_seams_and_image_edges(cuda_dev):
    H = W = 64
    spots = [(31, 31), (32, 32), (0, 0), (H - 1, W - 1)]
    imgs = []
    for (y, x) in spots:
        a = np.zeros((H, W, 3), dtype=np.uint8)
        a[y, x] = 255
        imgs.append(a)
    c = ds.DeviceImageCache.from_arrays(imgs, cuda_dev)
    src = list(range(4))
    rows = np.stack([row_of(np.eye(3), blur=1.5)] * 4)
    v, eps, _ = measured_eps(imgs, src, rows, 0, H, W)
    bits = launch(c, src, rows, 0, H, W, cuda_dev)
    assert_consistent(bits, v, eps, "blur of single pixels")
    o = _f64(bits[..., 0])
    for n, (y, x) in enumerate(spots):
        yy, xx = np.nonzero(o[n])
        assert max(abs(yy - y).max(), abs(xx - x).max()) == 4              # the 9-tap window, whole, across the seam at 32
        assert o[n, y, x] == o[n].max()
        for d in range(1, 5):                                              # mirror images about the pixel, bit for bit
            if 0 <= x - d and x + d < W:
                assert np.array_equal(bits[n, :, x - d], bits[n, :, x + d])
            if 0 <= y - d and y + d < H:
                assert np.array_equal(bits[n, y - d], bits[n, y + d])
        lo_y, lo_x = max(y - 4, 0), max(x - 4, 0)
        patch = o[n, lo_y:y + 5, lo_x:x + 5]
        assert np.abs(patch - patch.T).max() <= 2.0 ** -9 * patch.max()     # rows-then-columns against its transpose: one bf16 step
    assert abs(o[0].sum() - 1.0) < 0.02 and abs(o[1].sum() - 1.0) < 0.02   # the interior spread keeps the pixel's mass


# ------------------------------------------------------------------------------------------------ noise
def test_noise_is_a_function_of_seed_slot_and_pixel(cuda_dev):
    H = W = 64
    black = [np.zeros((H, W, 3), dtype=np.uint8)]
    c = ds.DeviceImageCache.from_arrays(black, cuda_dev)
    rows = np.stack([row_of(np.eye(3), noise=1.0)] * 2)
    seed = (0x1234 << 32) | 0x9abcdef1
    a = launch(c, [0, 0], rows, seed, H, W, cuda_dev)
    assert np.array_equal(a, launch(c, [0, 0], rows, seed, H, W, cuda_dev))         # the same call, the same bits
    other = launch(c, [0, 0], rows, seed + 1, H, W, cuda_dev)
    high = launch(c, [0, 0], rows, seed + (1 << 32), H, W, cuda_dev)
    assert not np.array_equal(a, other) and not np.array_equal(a, high) and not np.array_equal(a[0], a[1])
    # the integer hash, read back: on a black image with sigma 1 the output is max(z, 0) / 255 of the pixel's own z -- 4096
    # coordinates of slot 0 and 4096 of slot 1 against the oracle's hash and Box-Muller
    v, eps, m = measured_eps(black, [0, 0], rows, seed, H, W)
    assert_consistent(a, v, eps, "noise on black (oracle float32 vs float64: %.3g)" % m)
    assert_consistent(high, ref.augment(black, [0, 0], rows, seed + (1 << 32), H, W), eps, "noise, high seed word")
    positive = (a[0, :, :, 0] != 0).mean()
    assert 0.45 < positive < 0.55 and np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2])
    z = ref.normal(seed, 0, H, W)
    assert abs(z.mean()) < 0.06 and abs(z.std() - 1) < 0.05                          # and it is a standard normal field


# ------------------------------------------------------------------------------------------------ neutral parameters
@pytest.mark.parametrize("H,W", SHAPES)
def test_neutral_photometric_parameters_are_the_geometry_only_result(cuda_dev, cache, H, W):
    rows = rows_for(IMAGES, SRC, H, W, "all")
    want = launch(cache, SRC, rows, 0, H, W, cuda_dev)
    other = rows.copy()
    other[:, 8] = [0.0, 3.0, 255.0, 1e9]          # gamma_max: any
    other[:, 9] = [0.0, -0.0, -1.0, 0.0]          # no blur
    assert np.array_equal(launch(cache, SRC, other, 12345, H, W, cuda_dev), want)


def test_a_source_index_outside_the_cache_reads_nothing(cuda_dev, cache):
    rows = rows_for(IMAGES, [0, 0], 40, 72)
    bits = launch(cache, [-1, len(IMAGES)], rows, 0, 40, 72, cuda_dev)
    grey = launch(cache, [1], row_of(np.array([[1.0, 0, 1000], [0, 1.0, 0], [0, 0, 1]]))[None], 0, 40, 72, cuda_dev)
    assert np.array_equal(bits[0], grey[0]) and np.array_equal(bits[1], grey[0]) and len(np.unique(grey[..., :3])) == 1


# ------------------------------------------------------------------------------------------------ streams
def test_side_stream_and_graph_replay_give_the_eager_result(cuda_dev, photo_cache):
    H, W = 40, 72
    rows = rows_for(PHOTO_IMAGES, PHOTO_SRC, H, W, "all", **PHOTO["together"])
    want = launch(photo_cache, PHOTO_SRC, rows, 9, H, W, cuda_dev)
    src_t = torch.tensor(PHOTO_SRC, dtype=torch.int32, device=cuda_dev)
    rows_t = torch.from_numpy(rows).to(cuda_dev)
    out = poisoned(4, H, W, cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    s = torch.cuda.Stream(cuda_dev)
    with torch.cuda.stream(s):
        ops.letterbox_augment(photo_cache, src_t, rows_t, 9, H, W, out=out)
    s.synchronize()
    assert np.array_equal(out.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        ops.letterbox_augment(photo_cache, src_t, rows_t, 9, H, W, out=out)
    for _ in range(2):
        out.copy_(poisoned(4, H, W, cuda_dev))
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        assert np.array_equal(out.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF, want)
    # new parameters at the same pointers: the replay reads them, nothing was baked in at capture
    rows2 = rows_for(PHOTO_IMAGES, PHOTO_SRC, H, W, "rot5", **PHOTO["gray03"])
    rows_t.copy_(torch.from_numpy(rows2))
    g.replay()
    torch.cuda.synchronize(cuda_dev)
    assert np.array_equal(out.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF, launch(photo_cache, PHOTO_SRC, rows2, 9, H, W, cuda_dev))


def test_wrapper_refuses_what_the_kernel_cannot_take(cuda_dev, cache):
    rows = torch.from_numpy(rows_for(IMAGES, SRC, 64, 64)).to(cuda_dev)
    src = torch.tensor(SRC, dtype=torch.int32, device=cuda_dev)
    with pytest.raises(RuntimeError, match="params"):
        ops.letterbox_augment(cache, src, rows[:, :15].contiguous(), 0, 64, 64)
    with pytest.raises(RuntimeError, match="src_index"):
        ops.letterbox_augment(cache, src.long(), rows, 0, 64, 64)
    with pytest.raises(RuntimeError, match="out"):
        ops.letterbox_augment(cache, src, rows, 0, 64, 64, out=torch.empty((4, 64, 64, 8), device=cuda_dev))
    with pytest.raises(RuntimeError, match="GPU"):
        ds.DeviceImageCache.from_arrays(IMAGES, "cpu")
    assert math.isclose(cache.maxima[2], float(IMAGES[2].max())) and cache.nbytes == sum(a.nbytes for a in IMAGES)
