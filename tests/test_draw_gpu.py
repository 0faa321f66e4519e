"""GPU tier: ryolo_draw_quads (csrc/draw.hip) and ryolo_det_corners (csrc/detpost.hip) against tests/draw_reference.py, bit for bit:
every byte of dst is compared, the guard bytes between and after the images included; no pixel is excluded, no tolerance applies.

One pixel buffer holds images of (1, 1), (37, 53), (70, 130), (64, 64) and (33, 200) at byte offsets of every residue mod 4 with guard
bytes between them: several 64 x 64 tiles in both directions, ragged right and bottom edges, rows of every alignment.  dst is poisoned
before each call."""
import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.model import hip_ops as ops
from tests import detect_reference as dref
from tests import draw_reference as ref

pytestmark = pytest.mark.gpu

HW = [(1, 1), (37, 53), (70, 130), (64, 64), (33, 200)]
RESIDUE = [0, 1, 2, 3, 1]
POISON = 0xA5


def layout():
    offs, pos = [], 0
    for (h, w), res in zip(HW, RESIDUE):
        pos += 1 if offs else 0                          # at least one guard byte after the previous image
        while pos % 4 != res:
            pos += 1
        offs.append(pos)
        pos += 3 * h * w
    return offs, pos + 7


OFFS, NBYTES = layout()


@pytest.fixture(scope="module")
def scene(cuda_dev):
    """the source bytes (random, guard bytes too) on the host and on the device, with the layout tensors"""
    assert sorted(o % 4 for o in OFFS) == [0, 1, 1, 2, 3]
    src = np.random.default_rng(7).integers(0, 256, NBYTES, dtype=np.uint8)
    dev = (torch.from_numpy(src).to(cuda_dev), torch.tensor(OFFS, dtype=torch.int64, device=cuda_dev),
           torch.tensor(HW, dtype=torch.int32, device=cuda_dev), HW)
    return src, dev


def shapes(h, w):
    """axis-aligned, at 45 degrees, a nearly vertical sliver, four equal corners (a disc), two pairs of equal corners (a line)"""
    cx, cy, r = w // 2, h // 2, max(min(h, w) // 3, 1)
    return [[2, 2, 2, h - 3, w - 3, h - 3, w - 3, 2], [cx - r, cy, cx, cy + r, cx + r, cy, cx, cy - r], [5, 1, 6, h - 2, 7, h - 2, 6, 1],
            [w // 3, h // 3] * 4, [3, h - 2, 3, h - 2, w - 2, 4, w - 2, 4]]


def colors_for(m, seed=1):
    c = np.random.default_rng(seed).integers(0, 256, (m, 4), dtype=np.uint8)
    c[:, 3] = 0
    return c


def run(scene, cuda_dev, per_image, thick, labels=None, colors=None, in_place=False, check_inputs=False):
    """per_image: for each of the five images its list of quads.  Draws on the device into a poisoned dst and on the host with the oracle,
    compares every byte, and returns the drawn bytes."""
    src, (pixels, offs, hw, host_hw) = scene
    quad = np.array([q for rows in per_image for q in rows], dtype=np.int32).reshape(-1, 8)
    det_off = np.concatenate(([0], np.cumsum([len(r) for r in per_image]))).astype(np.int32)
    m = len(quad)
    colors = colors_for(m) if colors is None else colors
    thick = [thick] * len(HW) if np.isscalar(thick) else list(thick)
    q_t, off_t, c_t = torch.from_numpy(quad).to(cuda_dev), torch.from_numpy(det_off).to(cuda_dev), torch.from_numpy(colors).to(cuda_dev)
    lab_t = None if labels is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda_dev) for a in labels)
    if in_place:
        out = pixels.clone()
        start = src
    else:
        out = torch.full_like(pixels, POISON)
        start = np.full(NBYTES, POISON, dtype=np.uint8)
    got = ops.draw_quads((pixels if not in_place else out, offs, hw, host_hw), q_t, off_t, c_t, thick, labels=lab_t, out=out)
    torch.cuda.synchronize(cuda_dev)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    want = ref.draw(src, OFFS, HW, quad, det_off, colors, thick, labels, dst=start)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes differ, the first at %d (got %d, want %d)" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    if not in_place:
        assert np.array_equal(pixels.cpu().numpy(), src)
    if check_inputs:
        assert np.array_equal(q_t.cpu().numpy(), quad) and np.array_equal(c_t.cpu().numpy(), colors)
        assert np.array_equal(off_t.cpu().numpy(), det_off)
        if labels is not None:
            assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(lab_t, labels))
    return got


def image_of(flat, b):
    h, w = HW[b]
    return flat[OFFS[b]:OFFS[b] + 3 * h * w].reshape(h, w, 3)


@pytest.mark.parametrize("t", [1, 2, 3, 4, 7, 255])
def test_thickness_on_five_shapes(cuda_dev, scene, t):
    for k in range(5):                                   # one shape at a time on every image, then all of them over each other
        got = run(scene, cuda_dev, [[shapes(h, w)[k]] for h, w in HW], t)
        assert not np.array_equal(image_of(got, 2), image_of(scene[0], 2))
    run(scene, cuda_dev, [shapes(h, w) for h, w in HW], t)


def test_a_different_thickness_per_image(cuda_dev, scene):
    run(scene, cuda_dev, [shapes(h, w) for h, w in HW], [1, 2, 3, 4, 7])


def test_corners_left_of_above_and_beyond_the_image(cuda_dev, scene):
    per_image = [[[-20, -10, -25, h + 15, w + 30, h + 11, w + 40, -13], [-300, h // 2, w // 2, -200, w + 300, h // 2, w // 2, h + 200],
                  [-9, -9, -9, 5, 5, 5, 5, -9], [w - 5, h - 5, w - 5, h + 900, w + 1200, h + 900, w + 1200, h - 5]] for h, w in HW]
    got = run(scene, cuda_dev, per_image, 3)
    assert not np.array_equal(image_of(got, 1), image_of(scene[0], 1))


def test_a_quad_wholly_outside_paints_nothing(cuda_dev, scene):
    per_image = [[[w + 300, 5, w + 300, 50, w + 400, 50, w + 400, 5], [3, -700, 3, -600, 30, -600, 30, -700]] for h, w in HW]
    got = run(scene, cuda_dev, per_image, 7)
    for b in range(5):
        assert np.array_equal(image_of(got, b), image_of(scene[0], b))


def test_rows_out_of_the_coordinate_range_draw_nothing_label_included(cuda_dev, scene):
    per_image = [[[-16385, 2, 10, 2, 10, 12, 2, 12], [2, 2, 32768, 2, 10, 12, 2, 12], [2, 2, 10, 2, 10, 32768, 2, 12],
                  [2, -16385, 10, 2, 10, 12, 2, 12]] for _ in HW]
    m = 4 * len(HW)
    bits = np.ones(6 * 4, dtype=np.uint8)
    labels = (bits, np.zeros(m, dtype=np.int64), np.tile(np.array([[0, 0, 6, 4]], dtype=np.int32), (m, 1)))
    got = run(scene, cuda_dev, per_image, 4, labels=labels)
    for b in range(5):
        assert np.array_equal(image_of(got, b), image_of(scene[0], b))
    # the same rows just inside the range do draw
    per_image = [[[-16384, 2, 10, 2, 10, 12, 2, 12], [2, 2, 32767, 2, 10, 12, 2, 12]] for _ in HW]
    got = run(scene, cuda_dev, per_image, 4)
    assert not np.array_equal(image_of(got, 3), image_of(scene[0], 3))


def test_the_highest_row_wins_everywhere(cuda_dev, scene):
    per_image = [[[4, 4, 4, h - 6, w - 6, h - 6, w - 6, 4], [6, 2, 2, h - 4, w - 4, h - 8, w - 8, 6], [4, 4, 4, h - 6, w - 6, h - 6, w - 6, 4]]
                 for h, w in HW]
    colors = np.tile(np.array([[255, 0, 0, 0], [0, 255, 0, 0], [0, 0, 255, 0]], dtype=np.uint8), (len(HW), 1))
    got = run(scene, cuda_dev, per_image, 5, colors=colors)
    img = image_of(got, 3)
    assert (img == (0, 0, 255)).all(2).any() and not (img == (255, 0, 0)).all(2).any()    # row 0 lies wholly under row 2


def test_an_image_without_rows_between_two_with_rows_is_copied(cuda_dev, scene):
    per_image = [[], shapes(*HW[1]), [], shapes(*HW[3])[:2], []]
    got = run(scene, cuda_dev, per_image, 2)
    for b in (0, 2, 4):
        assert np.array_equal(image_of(got, b), image_of(scene[0], b))
    assert not np.array_equal(image_of(got, 1), image_of(scene[0], 1))


def test_no_rows_is_a_copy_and_in_place_nothing(cuda_dev, scene):
    got = run(scene, cuda_dev, [[] for _ in HW], 2)
    assert (got[OFFS[0] + 3:OFFS[1]] == POISON).all() and (got[-7:] == POISON).all()
    run(scene, cuda_dev, [[] for _ in HW], 2, in_place=True)


def test_more_rows_than_one_pass_holds(cuda_dev, scene):
    n = 4 * ops.DRAW_ROWS_PER_PASS + 3
    rng = np.random.default_rng(5)
    c = rng.integers(-4, 68, (n, 1, 2))
    quads = (c + rng.integers(-6, 7, (n, 4, 2))).reshape(n, 8).tolist()
    run(scene, cuda_dev, [[], [], [], quads, []], 2, colors=colors_for(n, seed=6))
    # sparse rows: most passes leave pixels unsettled, so every pass runs
    run(scene, cuda_dev, [[], quads[:5], [], [q if k % 97 == 0 else [900, 900] * 4 for k, q in enumerate(quads)], []], 1,
        colors=colors_for(n + 5, seed=6))


def label_set(rects, seed=3):
    """(lab_bits, lab_off, lab_rect) of random 0/1 bitmaps for rects = [(lx, ly, lw, lh)]"""
    rng = np.random.default_rng(seed)
    rect = np.array(rects, dtype=np.int32).reshape(-1, 4)
    sizes = rect[:, 2].astype(np.int64) * rect[:, 3]
    off = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    bits = (rng.random(int(sizes.sum())) < 0.6).astype(np.uint8) * rng.integers(1, 256, int(sizes.sum()), dtype=np.uint8)
    return bits, off, rect


def test_labels_sticking_out_on_every_side_outside_and_empty(cuda_dev, scene):
    per_image, rects = [], []
    for h, w in HW:
        per_image.append([[w // 2, h // 2, w // 2, h // 2 + 3, w // 2 + 3, h // 2 + 3, w // 2 + 3, h // 2]] * 7)
        rects += [(-5, 3, 12, 6), (w - 6, 2, 13, 5), (4, -3, 9, 7), (5, h - 4, 8, 9), (w + 10, h + 10, 6, 6), (3, 3, 0, 5), (-2, -2, w + 4, h + 4)]
    got = run(scene, cuda_dev, per_image, 1, labels=label_set(rects), check_inputs=True)
    assert not np.array_equal(image_of(got, 4), image_of(scene[0], 4))
    per_image = [rows[:6] for rows in per_image]
    rects = [r for k, r in enumerate(rects) if k % 7 != 6]
    run(scene, cuda_dev, per_image, 1, labels=label_set(rects))


def test_a_label_under_a_higher_outline_and_over_a_lower_one(cuda_dev, scene):
    per_image, rects = [], []
    for h, w in HW:
        box = [2, 2, 2, h - 3, w - 3, h - 3, w - 3, 2]
        per_image.append([box, box, box])
        rects += [(0, 0, min(w, 40), min(h, 12)), (0, 0, 0, 0), (1, 1, min(w, 30), min(h, 9))]
    colors = np.tile(np.array([[255, 0, 0, 0], [0, 255, 0, 0], [0, 0, 255, 0]], dtype=np.uint8), (len(HW), 1))
    run(scene, cuda_dev, per_image, 3, labels=label_set(rects), colors=colors)


def test_no_label_pointers_equal_labels_of_width_zero(cuda_dev, scene):
    per_image = [shapes(h, w) for h, w in HW]
    m = 5 * len(HW)
    a = run(scene, cuda_dev, per_image, 2)
    rect = np.tile(np.array([[3, 3, 0, 5]], dtype=np.int32), (m, 1))
    b = run(scene, cuda_dev, per_image, 2, labels=(np.ones(4, dtype=np.uint8), np.zeros(m, dtype=np.int64), rect))
    assert np.array_equal(a, b)


def test_in_place_gives_the_bytes_of_the_out_of_place_call(cuda_dev, scene):
    per_image = [shapes(h, w) for h, w in HW]
    rects = [(q[0], q[1] - 5, 11, 5) for rows in per_image for q in rows]
    a = run(scene, cuda_dev, per_image, 3, labels=label_set(rects), check_inputs=True)
    b = run(scene, cuda_dev, per_image, 3, labels=label_set(rects), in_place=True)
    for k in range(5):
        assert np.array_equal(image_of(a, k), image_of(b, k))


def test_side_stream_and_graph_replay(cuda_dev, scene):
    src, (pixels, offs, hw, host_hw) = scene
    per_image = [shapes(h, w) for h, w in HW]
    quad = np.array([q for rows in per_image for q in rows], dtype=np.int32)
    det_off = np.arange(0, 26, 5, dtype=np.int32)
    colors, thick = colors_for(25), [1, 2, 3, 4, 7]
    labels = label_set([(q[0], q[1] - 5, 11, 5) for q in quad.tolist()])
    want = ref.draw(src, OFFS, HW, quad, det_off, colors, thick, labels, dst=np.full(NBYTES, POISON, dtype=np.uint8))
    q_t, off_t, c_t = torch.from_numpy(quad).to(cuda_dev), torch.from_numpy(det_off).to(cuda_dev), torch.from_numpy(colors).to(cuda_dev)
    lab_t = tuple(torch.from_numpy(a).to(cuda_dev) for a in labels)
    out = torch.full_like(pixels, POISON)
    torch.cuda.synchronize(cuda_dev)
    s = torch.cuda.Stream(cuda_dev)
    with torch.cuda.stream(s):
        ops.draw_quads((pixels, offs, hw, host_hw), q_t, off_t, c_t, thick, labels=lab_t, out=out)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        ops.draw_quads((pixels, offs, hw, host_hw), q_t, off_t, c_t, thick, labels=lab_t, out=out)
    for _ in range(2):
        out.fill_(POISON)
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        assert np.array_equal(out.cpu().numpy(), want)


def test_wrapper_names_the_argument_it_refuses(cuda_dev, scene):
    _, (pixels, offs, hw, host_hw) = scene
    px = (pixels, offs, hw, host_hw)
    quad = torch.zeros(2, 8, dtype=torch.int32, device=cuda_dev)
    off = torch.tensor([0, 1, 1, 2, 2, 2], dtype=torch.int32, device=cuda_dev)
    col = torch.zeros(2, 4, dtype=torch.uint8, device=cuda_dev)
    for kw, text in ((dict(quad=quad.long()), "quad must"), (dict(quad=quad[:, :7]), "quad must"), (dict(det_off=off[:5]), "det_off must"),
                     (dict(det_off=off.long()), "det_off must"), (dict(color=col[:, :3]), "color must"), (dict(thick=0), "thick must"),
                     (dict(thick=[1, 2]), "thick must"), (dict(thick=2.5), "thick must"), (dict(thick=256), "thick must"),
                     (dict(labels=(col, off)), "labels must"), (dict(out=torch.zeros(5, dtype=torch.uint8, device=cuda_dev)), "out must"),
                     (dict(labels=(pixels, off.long(), torch.zeros(2, 4, dtype=torch.int32, device=cuda_dev))), "lab_off must")):
        a = dict(quad=quad, det_off=off, color=col, thick=2, labels=None, out=None)
        a.update(kw)
        with pytest.raises(RuntimeError, match=text):
            ops.draw_quads(px, a["quad"], a["det_off"], a["color"], a["thick"], labels=a["labels"], out=a["out"])
    with pytest.raises(RuntimeError, match="cache.pixels must"):
        ops.draw_quads((pixels.cpu(), offs, hw, host_hw), quad, off, col, 2)
    with pytest.raises(RuntimeError, match="cache.hw must"):
        ops.draw_quads((pixels, offs, hw, host_hw[:4]), quad, off, col, 2)


# ---- ryolo_det_corners

def test_corners_equal_the_float64_restatement(cuda_dev):
    det = dref.quad_boxes()
    keep = dref.comparable(det)
    print("det_corners: %d of %d boxes compared" % (keep.sum(), len(det)))
    assert keep.sum() >= 0.9 * len(det) and keep[:10].all()
    want, _ = ref.corners(det)
    before = det.copy()
    d = torch.from_numpy(det).to(cuda_dev)
    out = torch.full((len(det), 8), -(1 << 30), dtype=torch.int32, device=cuda_dev)
    got = ops.det_corners(d, out=out)
    torch.cuda.synchronize(cuda_dev)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(d.cpu().numpy(), before)
    got = got.cpu().numpy().astype(np.int64)
    assert (got != -(1 << 30)).all()
    assert np.array_equal(got[keep], want[keep]), np.argwhere((got != want).any(1) & keep)[:5]
    # the same coordinates as ryolo_det_quads, in another order
    quads = ops.det_quads(d).cpu().numpy().astype(np.int64)
    key = lambda a: np.sort(a.reshape(-1, 4, 2)[..., 0] * 100000 + a.reshape(-1, 4, 2)[..., 1], 1)  # noqa: E731
    assert np.array_equal(key(got), key(quads))


def test_corners_of_no_rows_and_of_one(cuda_dev):
    assert tuple(ops.det_corners(torch.zeros(0, 8, device=cuda_dev)).shape) == (0, 8)
    det = np.array([[10, 20, 7, 3, 0, 0.9, 1, 0]], dtype=np.float32)
    got = ops.det_corners(torch.from_numpy(det).to(cuda_dev)).cpu().numpy()
    assert got.tolist() == [[6, 18, 6, 21, 13, 21, 13, 18]]


def test_corners_wrapper_refuses_other_dtypes_and_layouts(cuda_dev):
    det = torch.zeros(4, 8, device=cuda_dev)
    for bad in (det.double(), det[:, :7], det.t().contiguous().t(), det.cpu()):
        with pytest.raises(RuntimeError, match="det must"):
            ops.det_corners(bad)
    with pytest.raises(RuntimeError, match="out must"):
        ops.det_corners(det, out=torch.zeros(4, 8, device=cuda_dev))
    with pytest.raises(RuntimeError, match="out must"):
        ops.det_corners(det, out=torch.zeros(3, 8, dtype=torch.int32, device=cuda_dev))
