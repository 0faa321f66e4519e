"""CPU tier: weighted-merge rotated NMS (nms_style 'MERGE') -- the float64 restatement (tests/rnms_merge_reference.py) against the oracle
and by hand, the premises the GPU tests (tests/test_rnms_merge_gpu.py) rest on, and the surfaces that need no device: the style
argument, the entry points' flags, the header and the library's exports."""
import os
import re

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from oracle import riou
from rotate_yolov3_amd.utils.nms import nms as nms_mod
from tests import rnms_merge_reference as R
from tests.test_cabi import ROOT, _binding, _declared

NEW = ["ryolo_rnms_merge_segmented", "ryolo_rnms_merge_segmented_workspace_bytes"]


def _sorted(d):
    return d[np.argsort(-d[:, 5], kind="stable")]


INPUTS = [("clustered", 65, 9, 0.3), ("clustered", 700, 40, 0.3), ("clustered", 700, 40, 0.5), ("random", 700, 3, 0.3), ("random", 700, 3, 0.5)]


def _input(kind, n, k):
    return R.clustered(n, k, 7) if kind == "clustered" else _sorted(riou.random_boxes(n, seed=k))


@pytest.mark.parametrize("kind,n,k,thr", INPUTS)
def test_the_loop_keeps_what_the_oracle_keeps_and_owners_are_first_kept_overlaps(kind, n, k, thr):
    d = _input(kind, n, k)
    iou = riou.riou_matrix(d, d)
    r = R.merge_loop(d, thr, iou)
    assert np.array_equal(np.nonzero(r["keep"])[0], np.sort(riou.rnms(d, thr)))
    # the definition of include/ryolo.h, evaluated directly: the smallest kept i < j with IoU(i, j) > thr
    over = iou > np.float32(thr)
    for j in range(n):
        if r["keep"][j]:
            assert r["owner"][j] == j
        else:
            cand = np.nonzero(r["keep"][:j] & over[:j, j])[0]
            assert len(cand) and r["owner"][j] == cand[0]
    assert r["size"].sum() == n and np.array_equal(np.bincount(r["owner"], minlength=n), r["size"])


def test_premises_of_the_gpu_test():
    """every tile form of the owner pass occurs: dense tiles (more than 7 suppressing pairs) in the clustered input, listed (1..7) and
    empty ones in the random input; and the clustered inputs hold members whose angle is folded by pi"""
    d = R.clustered(700, 40, 7)
    for thr in (0.3, 0.5):
        assert max(R.tile_pair_counts(d, thr).values()) > 7
        r = R.merge_loop(d, thr)
        assert r["folded"] >= 1 and (r["size"] > 1).sum() > 10
    counts = list(R.tile_pair_counts(_sorted(riou.random_boxes(700, seed=3)), 0.3).values())
    assert any(1 <= c <= 7 for c in counts) and any(c == 0 for c in counts)
    # the stated figures of the inputs (seed 7)
    r = R.merge_loop(R.clustered(65, 9, 7), 0.3)
    assert (r["keep"].sum(), (r["size"] > 1).sum(), r["size"].max()) == (11, 10, 13)
    r = R.merge_loop(d, 0.3)
    assert (r["keep"].sum(), (r["size"] > 1).sum(), r["size"].max(), r["folded"]) == (64, 53, 25, 5)


def test_hand_cases():
    box = [100.0, 80.0, 40.0, 20.0, 0.3]
    # three coincident boxes: the mean is the box (up to the rounding of the weighted sum)
    d = np.array([box + [0.9], box + [0.6], box + [0.3]], np.float32)
    r = R.merge_loop(d, 0.5, iou=np.ones((3, 3), np.float32))
    assert r["keep"].tolist() == [True, False, False] and r["owner"].tolist() == [0, 0, 0]
    assert np.allclose(r["merged"][0], d[0, :5].astype(np.float64), rtol=1e-15, atol=0) and not r["merged"][1:].any()
    # three boxes differing in cx only: the weighted mean by hand
    d = np.array([[100, 80, 40, 20, 0.25, 0.5], [104, 80, 40, 20, 0.25, 0.25], [92, 80, 40, 20, 0.25, 0.25]], np.float32)
    r = R.merge_loop(d, 0.3)
    assert r["owner"].tolist() == [0, 0, 0]
    assert r["merged"][0].tolist() == [(0.5 * 100 + 0.25 * 104 + 0.25 * 92) / 1.0, 80.0, 40.0, 20.0, 0.25]
    # a chain A - B - C: B overlaps both, A and C do not overlap: B belongs to A, C is kept alone
    d = np.array([[100, 80, 40, 20, 0, 0.9], [125, 80, 40, 20, 0, 0.8], [150, 80, 40, 20, 0, 0.7]], np.float32)
    iou = riou.riou_matrix(d, d)
    assert iou[0, 1] > 0.2 and iou[1, 2] > 0.2 and iou[0, 2] == 0
    r = R.merge_loop(d, 0.2, iou)
    assert r["keep"].tolist() == [True, False, True] and r["owner"].tolist() == [0, 0, 2] and r["size"].tolist() == [2, 0, 1]
    assert r["merged"][2].tolist() == d[2, :5].astype(np.float64).tolist()
    assert abs(r["merged"][0][0] - (0.9 * 100 + np.float64(np.float32(0.8)) * 125) / (np.float64(np.float32(0.9)) + np.float64(np.float32(0.8)))) < 1e-5
    # two near-identical boxes at +1.55 and -1.55: the same box up to 0.04 rad; the plain mean would turn it by 90 degrees
    d = np.array([[100, 80, 40, 20, 1.55, 0.9], [100.5, 80, 40, 20, -1.55, 0.8]], np.float32)
    r = R.merge_loop(d, 0.3)
    assert r["owner"].tolist() == [0, 0] and r["folded"] == 1
    assert abs(r["merged"][0][4] - 1.55) < 0.05
    # a group whose scores are all 0: the owner's own fields
    d = np.array([box + [0.0], box + [0.0]], np.float32)
    r = R.merge_loop(d, 0.5, iou=np.ones((2, 2), np.float32))
    assert r["merged"][0].tolist() == d[0, :5].astype(np.float64).tolist()


def test_an_unknown_style_is_a_value_error_before_any_device_work():
    pred = torch.zeros(1, 4, 7)
    for bad in ("AND", "SOFT", "merge", None):
        for fn in (nms_mod.non_max_suppression, nms_mod.non_max_suppression_batched):
            with pytest.raises(ValueError, match="'OR'.*'MERGE'"):
                fn(pred, 0.5, 0.5, nms_style=bad)
        with pytest.raises(ValueError, match="'OR'.*'MERGE'"):
            nms_mod.nms_from_candidates(torch.zeros(1, dtype=torch.long), torch.zeros(1, 8), 1, 0.5, nms_style=bad)
    assert nms_mod.non_max_suppression(pred, 0.5, 0.5, nms_style="MERGE") == [None]          # nothing passes the filter: no NMS call


def test_entry_point_flags():
    import detect
    import test as test_py
    for mod in (detect, test_py):
        parser, _ = mod.build_parser()
        assert parser.parse_args([]).nms_style == "OR"
        assert parser.parse_args(["--nms-style", "MERGE"]).nms_style == "MERGE"
        with pytest.raises(SystemExit):
            parser.parse_args(["--nms-style", "SOFT"])


def test_header_declares_and_library_exports_the_merge_entry():
    names = _declared()
    assert all(n in names for n in NEW)
    lib = _binding()
    for n in NEW:
        assert getattr(lib, n) is not None
    assert lib.ryolo_abi_version() == 4
    seg = lib.ryolo_rnms_segmented_workspace_bytes(700, 2, 400)
    assert lib.ryolo_rnms_merge_segmented_workspace_bytes(700, 2, 400) == seg + 512        # 2 x 7 keep words, 2 x 28 tile marks: a 256-byte unit each
    assert lib.ryolo_rnms_merge_segmented_workspace_bytes(0, 2, 400) == 0
    # argument checks come before anything is enqueued (no device needed): the addresses below are never read
    big = 1 << 30
    assert lib.ryolo_rnms_merge_segmented(64, 5, 6, 64, 1, 5, 0.5, 64, None, 64, 64, big, None) == -1        # NULL owner
    assert lib.ryolo_rnms_merge_segmented(64, 5, 6, 64, 1, 5, 0.5, 64, 64, None, 64, big, None) == -1        # NULL merged
    assert lib.ryolo_rnms_merge_segmented(64, 5, 5, 64, 1, 5, 0.5, 64, 64, 64, 64, big, None) == -1          # row stride below 6
    assert lib.ryolo_rnms_merge_segmented(64, 5, 6, 64, 1, 5, 0.5, 64, 64, 64, 64, 16, None) == -1           # workspace too small
    assert lib.ryolo_rnms_merge_segmented(64, 0, 6, 64, 1, 5, 0.5, 64, 64, 64, 64, big, None) == 0           # nothing to do
    doc = open(os.path.join(ROOT, "rotate-yolov3_amd", "utils", "nms", "nms.py")).read()
    assert re.search(r"'AND' and 'SOFT' styles.*not reproduced", doc, re.S)
