"""CPU tier: the drawing feature without a GPU -- the C ABI's declarations and argument rules (ryolo_det_corners, ryolo_draw_quads), the
oracle's own properties (tests/draw_reference.py), the host side of utils/plots.py and detect.py's --save-img guard."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.utils import plots
from tests import draw_reference as ref

EINVAL = -1      # RYOLO_EINVAL
P = 1 << 20          # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused before any HIP call


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), os.pardir, "include", "ryolo.h")).read()
    L = _lib.lib()
    for name, nargs in (("ryolo_det_corners", 4), ("ryolo_draw_quads", 16)):
        assert "int %s(" % name in header
        assert name in _lib._sigs and len(_lib._sigs[name][1]) == nargs
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert L.ryolo_abi_version() == 4
    assert L.ryolo_draw_rows_per_pass() == ops.DRAW_ROWS_PER_PASS
    assert L.ryolo_draw_max_images() >= 64


def draw_args(**kw):
    thick = kw.pop("thick_values", [2, 3])
    a = dict(src=P, dst=P + 4096, img_offset=P, img_hw=P, n_img=len(thick), max_h=64, max_w=64, quad=P, det_off=P, M=4, color=P,
             thick=(C.c_int * max(len(thick), 1))(*thick), lab_bits=None, lab_off=None, lab_rect=None, stream=None)
    a.update(kw)
    return [a[k] for k in ("src", "dst", "img_offset", "img_hw", "n_img", "max_h", "max_w", "quad", "det_off", "M", "color", "thick",
                           "lab_bits", "lab_off", "lab_rect", "stream")], a["thick"]


BAD = [dict(src=None), dict(dst=None), dict(img_offset=None), dict(img_hw=None), dict(thick=None), dict(n_img=0), dict(n_img=-1),
       dict(M=-1), dict(quad=None), dict(det_off=None), dict(color=None), dict(quad=P + 8), dict(quad=P + 4, M=0),
       dict(thick_values=[2, 0]), dict(thick_values=[256, 2]), dict(thick_values=[-1, 2]), dict(max_h=0), dict(max_w=0),
       dict(max_h=16385), dict(max_w=16385), dict(lab_bits=P), dict(lab_off=P, lab_rect=P), dict(lab_bits=P, lab_rect=P),
       dict(lab_bits=P, lab_off=P), dict(n_img=1 << 20)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % (k, "P+%d" % (v - P) if isinstance(v, int) and v >= P else v)
                                                            for k, v in d.items()))
def test_draw_quads_refuses_before_any_hip_call(bad):
    args, keep = draw_args(**bad)
    assert _lib.lib().ryolo_draw_quads(*args) == EINVAL


def test_draw_quads_of_no_rows_in_place_is_no_launch():
    # M == 0 with dst == src returns before any HIP call: it succeeds on a machine without a GPU, with pointers that are never read
    args, keep = draw_args(dst=P, M=0, quad=None, det_off=None, color=None)
    assert _lib.lib().ryolo_draw_quads(*args) == 0


def test_det_corners_argument_rules():
    L = _lib.lib()
    assert L.ryolo_det_corners(P, -1, P, None) == EINVAL
    assert L.ryolo_det_corners(None, 0, None, None) == 0
    assert L.ryolo_det_corners(None, 1, P, None) == EINVAL and L.ryolo_det_corners(P, 1, None, None) == EINVAL
    assert L.ryolo_det_corners(P + 4, 1, P, None) == EINVAL and L.ryolo_det_corners(P, 1, P + 8, None) == EINVAL


# ---- the oracle's own properties

def test_oracle_thin_horizontal_edge_paints_its_pixel_row():
    m = ref.covers([3, 5, 12, 5, 12, 5, 3, 5], 1, 11, 20)
    want = np.zeros((11, 20), dtype=bool)
    want[5, 3:13] = True
    assert np.array_equal(m, want)


def test_oracle_is_invariant_under_rotation_and_reversal_of_the_corners():
    rng = np.random.default_rng(2)
    for t in (1, 2, 3, 7):
        q = rng.integers(-5, 45, (4, 2))
        base = ref.covers(q.reshape(-1), t, 40, 40)
        assert base.any()
        for k in range(4):
            assert np.array_equal(ref.covers(np.roll(q, k, 0).reshape(-1), t, 40, 40), base)
            assert np.array_equal(ref.covers(np.roll(q[::-1], k, 0).reshape(-1), t, 40, 40), base)


def test_oracle_transposing_the_quad_transposes_the_mask():
    rng = np.random.default_rng(3)
    for t in (1, 2, 4, 9):
        q = rng.integers(-5, 50, (4, 2))
        assert np.array_equal(ref.covers(q[:, ::-1].reshape(-1), t, 45, 33), ref.covers(q.reshape(-1), t, 33, 45).T)


def test_oracle_corners_of_one_row_by_hand():
    q, _ = ref.corners(np.array([[10, 20, 7, 3, 0, 0.9, 1, 0]], dtype=np.float32))
    assert q.tolist() == [[6, 18, 6, 21, 13, 21, 13, 18]]


def test_oracle_largest_row_wins_and_out_of_range_rows_draw_nothing():
    img = np.zeros((20, 20, 3), dtype=np.uint8)
    quads = np.array([[2, 2, 2, 12, 12, 12, 12, 2], [2, 2, 2, 12, 12, 12, 12, 2], [2, 2, 2, 12, 12, 12, 32768, 2]])
    colors = np.array([[1, 2, 3, 0], [4, 5, 6, 0], [7, 8, 9, 0]], dtype=np.uint8)
    out = ref.draw_image(img, quads, colors, 1)
    assert set(map(tuple, out.reshape(-1, 3).tolist())) == {(0, 0, 0), (4, 5, 6)}


# ---- utils/plots.py on the host

def test_render_label_is_a_deterministic_bitmap_and_grows_with_the_text():
    a = plots.render_label("ship 0.93", 2)
    assert a.dtype == np.uint8 and a.ndim == 2 and a.any() and set(np.unique(a).tolist()) <= {0, 1}
    plots._LABELS.clear()
    b = plots.render_label("ship 0.93", 2)
    assert b is not a and np.array_equal(a, b)
    assert plots.render_label("ship 0.93", 2) is b                        # cached by (text, tl)
    assert plots.render_label("ship 0.93 and more", 2).shape[1] > a.shape[1]
    assert plots.render_label("ship 0.93", 4).shape[0] > a.shape[0]        # size max(10, 7 tl)


def test_pack_labels_anchors_the_bottom_left_at_corner_zero():
    bms = [np.ones((3, 5), dtype=np.uint8), None, np.arange(8, dtype=np.uint8).reshape(4, 2)]
    bits, off, rect = plots.pack_labels(bms, np.array([[10, 20], [7, 7], [-3, 2]]))
    assert bits.dtype == np.uint8 and off.dtype == np.int64 and rect.dtype == np.int32
    assert rect.tolist() == [[10, 17, 5, 3], [7, 7, 0, 0], [-3, -2, 2, 4]]
    assert off.tolist() == [0, 15, 15] and bits.tolist() == [1] * 15 + list(range(8))
    bits, off, rect = plots.pack_labels([], np.zeros((0, 2), dtype=np.int64))
    assert len(bits) == 0 and off.shape == (0,) and rect.shape == (0, 4)


def test_line_thickness_is_the_reference_formula():
    assert plots.line_thickness(64, 64) == 1
    assert plots.line_thickness(1536, 2048) == round(0.002 * (1536 + 2048) / 2) + 1 == 5
    assert plots.line_thickness(1250, 1250) == round(2.5) + 1 == 3       # a half-way case: Python's round goes to even
    assert plots.line_thickness(1750, 1750) == round(3.5) + 1 == 5


def test_class_colors_are_reproducible():
    a = plots.class_colors(7)
    assert a.dtype == np.uint8 and a.shape == (7, 3) and np.array_equal(a, plots.class_colors(7, seed=0))
    assert not np.array_equal(a, plots.class_colors(7, seed=1))


def test_label_text_and_class_names(tmp_path):
    assert plots.label_text(["ship", "car"], 1.0, 0.876) == "car 0.88" and plots.label_text(None, 3.0, 0.5) == "3 0.50"
    assert plots.label_text(["ship"], 2.0, 0.5) == "2 0.50"
    (tmp_path / "x.names").write_text("ship\ncar\n")
    (tmp_path / "x.data").write_text("classes=2\nnames=%s\n" % (tmp_path / "x.names"))
    assert plots.load_class_names(str(tmp_path / "x.data")) == ["ship", "car"]
    assert plots.load_class_names(str(tmp_path / "none.data")) is None


def test_mosaic_rows_put_the_targets_into_their_cells():
    t = np.array([[1, 0, 0.5, 0.25, 0.5, 0.125, 0.3], [0, 0, 0.5, 0.5, 1.0, 1.0, 0.0], [4, 0, 0.5, 0.5, 0.5, 0.5, 0.1],
                  [2, 0, 0.0, 1.0, 0.25, 0.25, -0.2]], dtype=np.float32)
    det = plots.mosaic_rows(t, 3, 2, 64, 32)
    assert det.dtype == np.float32 and det[:, :4].tolist() == [[16, 32, 32, 64], [48, 16, 16, 8], [0, 128, 8, 16]]
    assert det[:, 4].tolist() == [0.0, np.float32(0.3), np.float32(-0.2)]


def test_detect_save_img_refuses_the_source_folder_as_output(tmp_path):
    from PIL import Image
    import detect
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(str(tmp_path / "a.png"))
    opt = argparse.Namespace(hyp='', cfg='no such cfg', weights='', source=str(tmp_path), output=str(tmp_path / "." / ""), img_size=64,
                             conf_thres=0.5, nms_thres=0.3, batch_size=2, synthetic=2, save_img=True)
    with pytest.raises(ValueError, match="overwrite their sources"):
        detect.detect(opt)
    opt.source = str(tmp_path / "a.png")
    with pytest.raises(ValueError, match="overwrite their sources"):
        detect.detect(opt)
    assert sorted(os.listdir(str(tmp_path))) == ["a.png"]
