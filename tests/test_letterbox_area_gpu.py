"""GPU tier: ryolo_letterbox_area (csrc/letterbox_area.hip) against the float64 oracle tests/letterbox_area_reference.py.

The comparison rule is that of tests/test_letterbox_augment_gpu.py: an output o (bf16) must be the round-to-nearest-even bf16 of SOME
value in [v - eps, v + eps], v the oracle's float64 value in [0, 1] units; no pixel is excluded; every output buffer is pre-filled with
NaN bits.  eps is measured the way that file measures its photometric eps: 8 x the largest difference between the oracle evaluated in
float32 (the kernel's operations in the kernel's order) and in float64 on the test's own inputs.  It is printed, never tuned.  (For
scale: the longest chain of these shapes is (300, 7) -> 64 x 1, 6 + 8 products of magnitude <= 255 * 300 summed per pixel, each addition
half an ulp.  Measured on an MI355X run: the two precisions differ by 1.3e-7, eps = 1.0e-6 in [0, 1] units, against a bf16 spacing of 2^-8.)

The argument validation needs no GPU: tests/test_detect_images_cpu.py."""
import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model.nhwc_batch import NHWC8Batch
from rotate_yolov3_amd.utils import datasets as ds
from tests import letterbox_area_reference as ref
from tests.test_letterbox_augment_gpu import assert_consistent, poisoned

pytestmark = pytest.mark.gpu

_rng = np.random.default_rng(2017)
SIZES = ((37, 53), (64, 64), (1, 1), (90, 30), (200, 131), (128, 64), (300, 7))
IMAGES = [_rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
SRC = list(range(len(IMAGES))) + [-1]
SHAPES = [(64, 64), (40, 72)]          # (H, W): whole tiles; partial tiles on both axes


def grey_bits(dev):
    """the bits of 128 / 255, as ryolo_nchw_f32_to_nhwc_bf16 rounds the fp32 quotient"""
    x = torch.from_numpy(np.full((1, 3, 1, 1), np.float32(128) / np.float32(255), dtype=np.float32)).to(dev)
    return int(ops.nchw_f32_to_nhwc_bf16(x).view(torch.int16).cpu().numpy().astype(np.int64)[0, 0, 0, 0] & 0xFFFF)


def places(H, W):
    """letterbox placement (utils.datasets.place_rows) into the square that fits H x W, moved 5 columns right when there is room, plus the
    row of the slot that reads nothing"""
    size = min(H, W)
    rows = ds.place_rows(SIZES, size)
    rows[:, 0] += min(5, W - size)
    return np.concatenate((rows, np.array([[0, 0, 1, 1]], dtype=np.int32)), 0)


@pytest.fixture(scope="module")
def cache(cuda_dev):
    return ds.DeviceImageCache.from_arrays(IMAGES, cuda_dev)


_oracle = {}


def oracle(H, W):
    """(float64 oracle, measured eps, largest float32-float64 difference) of the standard batch at H x W, computed once"""
    if (H, W) not in _oracle:
        pl = places(H, W)
        v64 = ref.letterbox_area(IMAGES, SRC, pl, H, W, np.float64)
        v32 = ref.letterbox_area(IMAGES, SRC, pl, H, W, np.float32)
        m = float(np.abs(v32.astype(np.float64) - v64).max())
        v64.setflags(write=False)
        _oracle[(H, W)] = (v64, 8 * m, m)
    return _oracle[(H, W)]


def launch(cache, src, place, H, W, dev):
    out = poisoned(len(src), H, W, dev)
    batch = ops.letterbox_area(cache, torch.tensor(src, dtype=torch.int32, device=dev), place, H, W, out=out)
    assert isinstance(batch, NHWC8Batch) and batch.data.data_ptr() == out.data_ptr() and tuple(batch.shape) == (len(src), 3, H, W)
    torch.cuda.synchronize(dev)
    return bits_of(out)


def bits_of(t):
    return t.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def converter_bits(img_f32_hwc, dev):
    """what ryolo_nchw_f32_to_nhwc_bf16 makes of an fp32 [h, w, 3] image"""
    x = torch.from_numpy(np.ascontiguousarray(img_f32_hwc, dtype=np.float32)).permute(2, 0, 1)[None].contiguous().to(dev)
    return bits_of(ops.nchw_f32_to_nhwc_bf16(x))[0]


def test_the_set_minifies_magnifies_and_copies():
    kinds = set()
    for H, W in SHAPES:
        for (h, w), (_, _, nw, nh) in zip(SIZES, places(H, W)[:-1]):
            for s, n in ((w, nw), (h, nh)):
                kinds.add('minify' if n < s else ('copy' if n == s else 'magnify'))
    assert kinds == {'minify', 'copy', 'magnify'}


@pytest.mark.parametrize("H,W", SHAPES)
def test_against_the_float64_oracle(cuda_dev, cache, H, W):
    v, eps, m = oracle(H, W)
    print("%dx%d: oracle float32 vs float64 differ by at most %.3g -> eps %.3g" % (H, W, m, eps))
    assert 0 < eps < 2.0 ** -12
    assert_consistent(launch(cache, SRC, places(H, W), H, W, cuda_dev), v, eps, "letterbox_area %dx%d" % (H, W))


@pytest.mark.parametrize("H,W", SHAPES)
def test_border_is_128_exactly_and_the_edge_is_hard(cuda_dev, cache, H, W):
    pl = places(H, W)
    bits = launch(cache, SRC, pl, H, W, cuda_dev)
    grey = grey_bits(cuda_dev)
    outside = 0
    for n, (left, top, nw, nh) in enumerate(pl):
        mask = np.ones((H, W), dtype=bool)
        if SRC[n] >= 0:
            mask[top:top + nh, left:left + nw] = False
        outside += int(mask.sum())
        assert (bits[n][mask][:, :3] == grey).all() and not bits[n][mask][:, 3:].any(), "slot %d" % n
    assert outside > H * W            # the slot that reads nothing, and margins elsewhere
    assert (bits[len(SRC) - 1][..., :3] == grey).all()      # src_index -1: all 128


def test_same_size_is_the_pixel_itself_bit_for_bit(cuda_dev, cache):
    """n == s on both axes: u8 / 255 with the border 128, what ryolo_nchw_f32_to_nhwc_bf16 makes of it"""
    H, W = 40, 72
    place = np.array([[3, 2, 53, 37], [19, 0, 30, 40]], dtype=np.int32)       # (37, 53) whole; (90, 30): x copied, y minified
    bits = launch(cache, [0, 3], place, H, W, cuda_dev)
    want = np.full((H, W, 3), 128, dtype=np.float32)
    want[2:39, 3:56] = IMAGES[0]
    assert np.array_equal(bits[0], converter_bits(want / np.float32(255), cuda_dev))
    full = launch(cache, [1, 5], np.array([[0, 0, 64, 64], [0, 0, 64, 64]], dtype=np.int32), 64, 64, cuda_dev)
    assert np.array_equal(full[0], converter_bits(IMAGES[1].astype(np.float32) / np.float32(255), cuda_dev))


def test_two_to_one_is_the_mean_of_each_block_bit_for_bit(cuda_dev):
    img = np.random.default_rng(4).integers(0, 256, (128, 128, 3), dtype=np.uint8)
    c = ds.DeviceImageCache.from_arrays([img], cuda_dev)
    bits = launch(c, [0], np.array([[0, 0, 64, 64]], dtype=np.int32), 64, 64, cuda_dev)
    f = img.astype(np.float32)
    mean = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2]) / np.float32(4)      # exact in fp32
    assert np.array_equal(bits[0], converter_bits(mean / np.float32(255), cuda_dev))


def test_a_source_index_outside_the_cache_is_all_border(cuda_dev, cache):
    pl = np.array([[0, 0, 40, 40], [7, 3, 20, 30]], dtype=np.int32)
    bits = launch(cache, [-1, len(IMAGES)], pl, 40, 72, cuda_dev)
    assert (bits[..., :3] == grey_bits(cuda_dev)).all() and not bits[..., 3:].any()


def test_more_slots_than_one_launch_carries(cuda_dev, cache):
    """the placement rows travel in the kernel arguments, 64 slots per launch: 70 slots are two launches"""
    rows = places(40, 72)[:-1]
    src = [k % len(IMAGES) for k in range(70)]
    pl = np.stack([rows[s] for s in src])
    bits = launch(cache, src, pl, 40, 72, cuda_dev)
    one = launch(cache, SRC, places(40, 72), 40, 72, cuda_dev)
    for k, s in enumerate(src):
        assert np.array_equal(bits[k], one[s]), k


def test_side_stream_and_graph_replay_give_the_eager_result(cuda_dev, cache):
    H, W = 40, 72
    pl = places(H, W)
    want = launch(cache, SRC, pl, H, W, cuda_dev)
    src_t = torch.tensor(SRC, dtype=torch.int32, device=cuda_dev)
    out = poisoned(len(SRC), H, W, cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    s = torch.cuda.Stream(cuda_dev)
    with torch.cuda.stream(s):
        ops.letterbox_area(cache, src_t, pl, H, W, out=out)
    s.synchronize()
    assert np.array_equal(bits_of(out), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        ops.letterbox_area(cache, src_t, pl, H, W, out=out)
    for _ in range(2):
        out.copy_(poisoned(len(SRC), H, W, cuda_dev))
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        assert np.array_equal(bits_of(out), want)
    # new source indices at the same pointer: the replay reads them (the placement rows were captured with the launch)
    src_t.copy_(torch.tensor([-1] * len(SRC), dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize(cuda_dev)
    assert (bits_of(out)[..., :3] == grey_bits(cuda_dev)).all()


def test_wrapper_refuses_what_the_kernel_cannot_take(cuda_dev, cache):
    src = torch.tensor(SRC, dtype=torch.int32, device=cuda_dev)
    pl = places(64, 64)
    with pytest.raises(RuntimeError, match="place"):
        ops.letterbox_area(cache, src, pl[:, :3], 64, 64)
    with pytest.raises(RuntimeError, match="place"):
        ops.letterbox_area(cache, src, torch.from_numpy(pl).to(cuda_dev), 64, 64)
    with pytest.raises(RuntimeError, match="src_index"):
        ops.letterbox_area(cache, src.long(), pl, 64, 64)
    with pytest.raises(RuntimeError, match="out"):
        ops.letterbox_area(cache, src, pl, 64, 64, out=torch.empty((len(SRC), 64, 64, 8), device=cuda_dev))
    bad = pl.copy()
    bad[0, 0] = 64 - bad[0, 2] + 1           # one column past the right edge
    with pytest.raises(RuntimeError, match="ryolo_letterbox_area"):
        ops.letterbox_area(cache, src, bad, 64, 64)
