"""CPU tier of the image path of detect.py: the file listing of LoadImages, place_rows, the --multi-scale draw, --scales, the ICDAR writer,
the host-side argument validation of the three new entry points and the numpy restatements the GPU tests compare against."""
import os
import zipfile

import numpy as np
import pytest

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.utils import datasets as ds
from rotate_yolov3_amd.utils import icdar
from rotate_yolov3_amd.utils.detect_images import rescale_geometry
from tests import detect_reference as dref
from tests import letterbox_area_reference as lref

import detect

EINVAL = -1


def _touch(path):
    with open(path, 'wb') as f:
        f.write(b'x')
    return str(path)


# ------------------------------------------------------------------------------------------------ LoadImages: listing
def test_listing_of_a_directory_a_file_and_a_list(tmp_path):
    d = tmp_path / 'imgs'
    d.mkdir()
    for name in ('b.png', 'a.JPG', 'c.txt', 'notes.md', 'a10.bmp', 'a2.jpeg'):
        _touch(d / name)
    want = [str(d / n) for n in ('a.JPG', 'a10.bmp', 'a2.jpeg', 'b.png')]          # sorted by name, images only
    assert ds.list_images(str(d)) == want
    assert ds.list_images(str(d / 'b.png')) == [str(d / 'b.png')]
    lst = tmp_path / 'list.txt'
    lst.write_text('\n'.join([want[3], want[0], str(d / 'notes.md'), '']) + '\n')
    assert ds.list_images(str(lst)) == [want[3], want[0]]                          # the list's own order
    loader = ds.LoadImages(str(d), 96, 3, 'cpu')
    assert loader.files == want and len(loader) == 2 and loader.batch_size == 3


def test_listing_refuses_videos_streams_and_nothing(tmp_path):
    with pytest.raises(NotImplementedError, match="OpenCV"):
        ds.list_images('0')
    with pytest.raises(NotImplementedError, match="OpenCV"):
        ds.list_images('rtsp://camera/stream')
    with pytest.raises(NotImplementedError, match="OpenCV"):
        ds.list_images(_touch(tmp_path / 'clip.mp4'))
    d = tmp_path / 'mixed'
    d.mkdir()
    _touch(d / 'a.png')
    _touch(d / 'b.avi')
    with pytest.raises(NotImplementedError, match="video"):
        ds.list_images(str(d))
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match="No images"):
        ds.list_images(str(empty))
    with pytest.raises(FileNotFoundError):
        ds.list_images(str(tmp_path / 'nowhere'))


# ------------------------------------------------------------------------------------------------ place_rows
@pytest.mark.parametrize("size", [64, 96, 608])
def test_place_rows_are_the_letterbox_of_the_reference(size):
    shapes = [(37, 53), (64, 64), (1, 1), (90, 30), (200, 131), (128, 64), (300, 7), (1536, 2048), (480, 640)]
    rows = ds.place_rows(shapes, size)
    assert rows.dtype == np.int32 and rows.shape == (len(shapes), 4)
    for (h, w), (left, top, nw, nh) in zip(shapes, rows):
        lb = ds.letterbox_matrix(h, w, size)
        assert (left, top, nw, nh) == (lb.left, lb.top, lb.new_unpad[0], lb.new_unpad[1])
        assert max(nw, nh) == size and left >= 0 and top >= 0 and left + nw <= size and top + nh <= size
        # the reference pads to size on both sides of the picture: top + bottom, left + right
        bottom, right = int(round(lb.dh + 0.1)), int(round(lb.dw + 0.1))
        assert top + nh + bottom == size and left + nw + right == size


def test_place_rows_keep_one_pixel_of_a_side_that_rounds_away():
    (left, top, nw, nh), = ds.place_rows([(300, 1)], 64)
    assert (nw, nh) == (1, 64) and 0 <= left and left + nw <= 64


# ------------------------------------------------------------------------------------------------ --multi-scale, --scales
def test_multi_scale_draw_and_its_range():
    assert detect.multi_scale_range(608) == (448, 768)          # (round(19 / 1.5) + 1) * 32, (round(19 * 1.3) - 1) * 32
    assert detect.multi_scale_range(416) == ((round(13 / 1.5) + 1) * 32, (round(13 * 1.3) - 1) * 32)
    seen = set()
    for seed in range(40):
        sizes = detect.multi_scale_sizes(608, seed)
        assert sizes == detect.multi_scale_sizes(608, seed)     # a function of the seed
        assert len(sizes) == 2 and sizes[0] != sizes[1] and all(isinstance(s, int) and s % 32 == 0 and 448 <= s <= 768 for s in sizes)
        seen.update(sizes)
    assert seen == set(range(448, 769, 32))                     # both ends are drawn


def test_scales_validation():
    assert detect.parse_scales('416,608,800') == [416, 608, 800]
    assert detect.parse_scales(' 64 , 96') == [64, 96]
    for bad in ('', '600', '416,416', '0', '-32', '416;608', 'a,b'):
        with pytest.raises(ValueError, match="--scales"):
            detect.parse_scales(bad)


def test_what_counts_as_an_image_source(tmp_path):
    assert detect.is_image_source(str(tmp_path))
    assert detect.is_image_source(_touch(tmp_path / 'a.png')) and detect.is_image_source(_touch(tmp_path / 'l.txt'))
    assert not detect.is_image_source(_touch(tmp_path / 'x.npy')) and not detect.is_image_source(_touch(tmp_path / 'x.pt'))
    assert not detect.is_image_source(str(tmp_path / 'missing')) and not detect.is_image_source('data/tiny/test/none')
    # what the reference hands to OpenCV is an image source too, so that LoadImages refuses it; a video path that does not exist is not
    assert detect.is_image_source('0') and detect.is_image_source('rtsp://camera/stream') and detect.is_image_source(_touch(tmp_path / 'v.mp4'))
    assert not detect.is_image_source(str(tmp_path / 'missing.mp4'))
    assert ds.is_video_or_stream('0') and ds.is_video_or_stream('a/b.AVI') and not ds.is_video_or_stream('a/b.png')


# ------------------------------------------------------------------------------------------------ ICDAR files
def test_icdar_writer_and_zip(tmp_path):
    d = tmp_path / 'icdar'
    d.mkdir()
    p1 = icdar.write_icdar(str(d), '/some/where/img_12.jpg', [[6, 18, 14, 18, 14, 22, 6, 22], np.array([-2, -1, 4, -1, 4, 3, -2, 3])])
    p2 = icdar.write_icdar(str(d), 'b.v2.png', [])
    assert os.path.basename(p1) == 'res_img_12.txt' and os.path.basename(p2) == 'res_b.v2.txt'
    assert open(p1).read() == '6,18,14,18,14,22,6,22\n-2,-1,4,-1,4,3,-2,3\n' and open(p2).read() == ''
    with pytest.raises(ValueError):
        icdar.write_icdar(str(d), 'c.png', [[1, 2, 3]])
    z = icdar.zip_dir(str(d), str(tmp_path / 'icdar_result.zip'))
    with zipfile.ZipFile(z) as zf:
        assert zf.namelist() == ['res_b.v2.txt', 'res_c.txt', 'res_img_12.txt']
        assert zf.read('res_img_12.txt') == open(p1, 'rb').read()
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in zf.infolist())
    # the files of one run only, whatever else lies in the folder
    z = icdar.zip_files([p2, p1], str(tmp_path / 'run.zip'))
    with zipfile.ZipFile(z) as zf:
        assert zf.namelist() == ['res_b.v2.txt', 'res_img_12.txt'] and zf.read('res_img_12.txt') == open(p1, 'rb').read()
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in zf.infolist())
    other = tmp_path / 'other'
    other.mkdir()
    with pytest.raises(ValueError, match="share a name"):
        icdar.zip_files([p1, _touch(other / 'res_img_12.txt')], str(tmp_path / 'twice.zip'))


# ------------------------------------------------------------------------------------------------ the C ABI, host side
def test_header_declares_and_library_exports_the_three_functions():
    for name in ('ryolo_letterbox_area', 'ryolo_det_rescale', 'ryolo_det_quads'):
        assert name in _lib._sigs and hasattr(_lib.lib(), name)
    assert len(_lib._sigs['ryolo_letterbox_area'][1]) == 11 and len(_lib._sigs['ryolo_det_rescale'][1]) == 6
    assert len(_lib._sigs['ryolo_det_quads'][1]) == 4


def test_letterbox_area_argument_validation_without_gpu():
    """every refusal comes before any HIP call: the pointers are never followed but for the placement rows, which are host memory"""
    L = _lib.lib()
    P = 4096                                     # a non-null, 16-byte aligned address nothing reads
    place = np.array([[0, 0, 64, 64], [21, 0, 21, 64]], dtype=np.int32)

    def call(pixels=P, offs=P, hw=P, n_cache=1, src=P, pl=place, N=2, H=64, W=64, y=P):
        return L.ryolo_letterbox_area(pixels, offs, hw, n_cache, src, None if pl is None else pl.ctypes.data, N, H, W, y, None)

    for kw in (dict(pixels=None), dict(offs=None), dict(hw=None), dict(src=None), dict(pl=None), dict(y=None), dict(n_cache=0), dict(N=0),
               dict(H=0), dict(W=-1), dict(y=P + 8), dict(H=65535 * 32 + 1)):
        assert call(**kw) == EINVAL, kw
    for row in ([0, 0, 0, 64], [0, 0, 64, 0], [-1, 0, 64, 64], [0, -1, 10, 10], [1, 0, 64, 64], [0, 1, 64, 64], [60, 0, 5, 5],
                [0, 2 ** 31 - 1, 1, 2 ** 31 - 1]):
        bad = place.copy()
        bad[1] = row
        assert call(pl=bad) == EINVAL, row
    many = np.tile(place[:1], (65536, 1))
    assert call(pl=many, N=65536) == EINVAL


def test_detpost_argument_validation_without_gpu():
    L = _lib.lib()
    P = 4096
    assert L.ryolo_det_rescale(None, 0, None, 1, None, None) == 0 and L.ryolo_det_quads(None, 0, None, None) == 0      # M == 0: no launch
    assert L.ryolo_det_rescale(P, -1, P, 1, P, None) == EINVAL and L.ryolo_det_rescale(P, 0, P, 0, P, None) == EINVAL
    for args in ((None, 1, P, 1, P), (P, 1, None, 1, P), (P, 1, P, 1, None), (P + 4, 1, P, 1, P)):
        assert L.ryolo_det_rescale(*args, None) == EINVAL, args
    assert L.ryolo_det_quads(P, -1, P, None) == EINVAL
    for args in ((None, 1, P), (P, 1, None), (P + 8, 1, P), (P, 1, P + 4)):
        assert L.ryolo_det_quads(*args, None) == EINVAL, args


# ------------------------------------------------------------------------------------------------ the restatements
def test_quads_restatement_on_four_hand_computed_boxes():
    a = float(np.arctan2(3.0, 4.0))              # cos 0.8, sin 0.6
    det = np.array([[10, 20, 8, 4, 0.0, 1, 1, 0],
                    [10, 20, 7, 3, np.pi / 2, 1, 1, 0],
                    [50, 50, 21, 11, a, 1, 1, 0],
                    [1, 1, 7, 5, 0.0, 1, 1, 0]])
    q, xy = dref.quads(det)
    assert q.tolist() == [[6, 18, 14, 18, 14, 22, 6, 22],
                          [8, 16, 11, 16, 11, 23, 8, 23],
                          [44, 39, 61, 51, 55, 60, 38, 48],
                          [-2, -1, 4, -1, 4, 3, -2, 3]]
    assert np.allclose(xy[2], [44.9, 39.3, 61.7, 51.9, 55.1, 60.7, 38.3, 48.1], atol=1e-9)


def test_order_points_ties():
    sq = np.array([[0.0, 0.0], [0.0, 2.0], [2.0, 2.0], [2.0, 0.0]])
    assert dref.order_points(sq).tolist() == [[0, 0], [2, 0], [2, 2], [0, 2]]
    # the two right-most equally far from tl: the later one is br
    pts = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 4.0], [4.0, 3.0]])
    assert dref.order_points(pts).tolist() == [[0, 0], [3, 4], [4, 3], [0, 0]]


def test_rescale_restatement_and_geometry():
    g = rescale_geometry([(64, 64), (97, 400), (1536, 2048)], 96)
    assert g.dtype == np.float32
    assert np.array_equal(g, np.array([[1.5, 0, 0], [0.24, 0, (96 - 97 * 0.24) / 2], [96 / 2048, 0, (96 - 1536 * (96 / 2048)) / 2]],
                                      dtype=np.float32))
    det = np.array([[30, 45, 9, 3.75, 0.3, 0.9, 1, 0], [48, 48, 2.25, 24, -0.2, 0.8, 1, 0]], dtype=np.float32)
    out = dref.rescale(det, [0, 1, 2], g[[0, 2]])
    assert out[0].tolist() == [20, 30, 6, 2, np.float32(0.3), np.float32(0.9), 1, 0]               # 2.5 rounds to even
    assert out[1].tolist() == [1024, 768, 48, 512, np.float32(-0.2), np.float32(0.8), 1, 0]


def test_the_quad_test_boxes_keep_nine_in_ten():
    det = dref.quad_boxes()
    keep = dref.comparable(det)
    assert keep.sum() >= 0.9 * len(det) and keep[:10].all()
    assert (det[:, 2:4] > 2).all() and np.array_equal(det[:, :4], np.rint(det[:, :4]))
    assert (det[0:10, 4] == 0).all() and (det[10:20, 4] == np.float32(np.pi / 2)).all() and (det[20:30, 4] == -np.float32(np.pi / 2)).all()
    assert (np.abs(det[30:, 4]) < np.pi / 2).all()


def test_area_taps_cover_exactly_and_centre_bilinear():
    for s, n in ((7, 3), (300, 64), (131, 42), (2048, 608), (5, 4)):
        total = np.zeros(s, dtype=np.int64)
        for k in range(n):
            idx, wts, D = lref.taps(k, s, n)
            assert D == s and sum(wts) == s and idx == list(range(idx[0], idx[0] + len(idx)))
            total[idx] += wts
        assert (total == n).all()                # every source pixel is spread over the outputs with total weight n / s ... times s
    assert lref.taps(5, 9, 9) == ([5, 6], [18, 0], 18)                       # n == s: the pixel itself
    assert lref.taps(0, 1, 64) == ([0, 0], [63, 65], 128)                    # clamped on both sides
    assert lref.taps(0, 2, 4) == ([0, 0], [2, 6], 8) and lref.taps(1, 2, 4) == ([0, 1], [6, 2], 8)     # centres at -0.25, 0.25
    img = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3) * 20
    out = lref.letterbox_area([img], [0, -1], [(1, 1, 2, 2), (0, 0, 1, 1)], 4, 4)
    assert np.array_equal(out[0, 1:3, 1:3], img / 255.0) and (out[1] == 128 / 255.0).all() and out[0, 0, 0, 0] == 128 / 255.0
