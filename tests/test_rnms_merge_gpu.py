"""GPU tier: weighted-merge rotated NMS (ryolo_rnms_merge_segmented, nms_style 'MERGE') against its float64 restatement
(tests/rnms_merge_reference.py; its premises are asserted in tests/test_rnms_merge_cpu.py).

Per case: keep_flags bit-equal to r_nms_segmented on the same tensor; owner equal to the reference exactly; for every kept row and field
|merged - float32(ref)| <= ulp32(ref) + 4 (m + 1) 2^-53 max_j |v_j| (m the group's size, v_j the members' field values, the angle after
folding) -- derived, not measured: two fp64 evaluations of the same quotient in different summation orders differ by at most the second
term, and rounding each to fp32 can then differ by one ulp; rows not kept exactly zero; a second call returns the same bits.  Every case
runs with one and with two column tiles per wave of the mask kernel (RYOLO_RNMS_TILES)."""
import functools

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from oracle import riou
from tests import rnms_merge_reference as R

pytestmark = pytest.mark.gpu

CLUSTERS = {1: 1, 2: 1, 63: 8, 64: 8, 65: 9, 129: 16, 700: 40}
SEGMENTS = [1, 64, 65, 200, 37]


@pytest.fixture(scope="module")
def ops(cuda_dev):
    from rotate_yolov3_amd.utils.nms import r_nms as m
    return m


@pytest.fixture(params=["1", "2"])
def tiles(request, ops):
    from rotate_yolov3_amd import _lib
    _lib.set_tuning("RYOLO_RNMS_TILES", request.param)
    yield request.param
    _lib.set_tuning("RYOLO_RNMS_TILES", None)


def _sorted(d):
    return d[np.argsort(-d[:, 5], kind="stable")]


@functools.lru_cache(maxsize=None)
def _single(kind, n):
    d = R.clustered(n, CLUSTERS[n], 7) if kind == "clustered" else _sorted(riou.random_boxes(n, seed=3))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _multi(kind):
    sets = [R.clustered(m, max(1, m // 16), 20 + k) if kind == "clustered" else _sorted(riou.random_boxes(m, seed=40 + k, extent=60.0))
            for k, m in enumerate(SEGMENTS)]
    d = np.concatenate(sets)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref_single(kind, n, thr):
    return R.segmented(_single(kind, n), (0, n), thr)


@functools.lru_cache(maxsize=None)
def _ref_multi(kind, thr):
    return R.segmented(_multi(kind), tuple(np.concatenate([[0], np.cumsum(SEGMENTS)]).tolist()), thr)


def _t(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)         # (a copy: the cached inputs are read-only)


def _check(ops, dev, d, offsets, thr, ref, dets=None):
    """all assertions of the module docstring for one call; returns (flags, merged, owner) as numpy arrays"""
    dets = _t(d, dev) if dets is None else dets
    off = torch.tensor(list(offsets), dtype=torch.int32, device=dev)
    max_len = int(np.diff(np.asarray(offsets)).max())
    flags, merged, owner = ops.r_nms_merge_segmented(dets, off, max_len, thr)
    assert flags.dtype == torch.uint8 and owner.dtype == torch.int32 and merged.dtype == torch.float32 and merged.shape == (len(d), 5)
    plain = ops.r_nms_segmented(dets, off, max_len, thr)
    assert torch.equal(flags, plain)
    f2, m2, o2 = ops.r_nms_merge_segmented(dets, off, max_len, thr)
    assert torch.equal(f2, flags) and torch.equal(o2, owner) and torch.equal(m2.view(torch.int32), merged.view(torch.int32))
    flags, merged, owner = flags.cpu().numpy().astype(bool), merged.cpu().numpy(), owner.cpu().numpy()
    assert np.array_equal(flags, ref["keep"])
    assert np.array_equal(owner, ref["owner"])
    assert not merged[~flags].any() and not np.signbit(merged[~flags]).any()
    want = ref["merged"].astype(np.float32).astype(np.float64)
    err = np.abs(merged.astype(np.float64) - want)[flags]
    bnd = R.bound(ref)[flags]
    print("n %d thr %g: kept %d, largest group %d, folded %d, largest error / bound %.3g"
          % (len(d), thr, flags.sum(), ref["size"].max(), ref["folded"], (err / bnd).max() if len(err) else 0.0))
    assert (err <= bnd).all()
    return flags, merged, owner


@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("kind", ["clustered", "random"])
@pytest.mark.parametrize("n", sorted(CLUSTERS))
def test_single_segment(ops, cuda_dev, tiles, n, kind, thr):
    _check(ops, cuda_dev, _single(kind, n), (0, n), thr, _ref_single(kind, n, thr))


@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("kind", ["clustered", "random"])
def test_ragged_segments_in_one_call(ops, cuda_dev, tiles, kind, thr):
    off = np.concatenate([[0], np.cumsum(SEGMENTS)]).tolist()
    flags, _, owner = _check(ops, cuda_dev, _multi(kind), off, thr, _ref_multi(kind, thr))
    seg_of = np.repeat(np.arange(len(SEGMENTS)), SEGMENTS)
    assert np.array_equal(seg_of[owner], seg_of)                      # an owner is a row of the same segment
    if kind == "clustered":
        assert (~flags).sum() > 100


def test_edge_cases(ops, cuda_dev, tiles):
    # a negative threshold (the mask kernel's rejects are off): every box overlaps the first, one owner with 130 members
    d = _sorted(riou.random_boxes(130, seed=32, extent=300.0))
    ref = R.segmented(d, (0, 130), -1.0)
    assert ref["size"][0] == 130 and ref["keep"].sum() == 1
    _check(ops, cuda_dev, d, (0, 130), -1.0, ref)
    # a box with w = 0: the IoU of its pairs is inf or NaN in the reference arithmetic; flags and owners follow the plain call and the loop
    z = R.clustered(65, 9, 7).copy()
    z[20, 2] = 0.0
    iou = riou.riou_matrix(z, z)
    assert not np.isfinite(iou[20]).all()
    _check(ops, cuda_dev, z, (0, 65), 0.3, R.segmented(z, (0, 65), 0.3))
    # one group whose scores are all 0 (the last rows: score order), next to groups with scores: the owner's own fields come back
    g = R.clustered(40, 3, 9).copy()
    box = np.array([900.0, 900.0, 40.0, 20.0, 0.3], np.float32)
    zero = np.zeros((3, 6), np.float32)
    zero[:, :5] = box + np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 1, 0, 0, 0]], np.float32)
    g = np.concatenate([g, zero])
    ref = R.segmented(g, (0, 43), 0.3)
    assert ref["keep"][40] and ref["size"][40] == 3
    _, merged, _ = _check(ops, cuda_dev, g, (0, 43), 0.3, ref)
    assert np.array_equal(merged[40], g[40, :5])
    # a strided dets ([m, 8] rows, columns 0..5) equals the contiguous call
    d = R.clustered(129, 16, 7)
    d8 = torch.cat([_t(d, cuda_dev), torch.full((129, 2), 7.0, device=cuda_dev)], 1)
    assert d8[:, :6].stride(0) == 8
    a = _check(ops, cuda_dev, d, (0, 129), 0.3, _ref_single("clustered", 129, 0.3))
    b = _check(ops, cuda_dev, d, (0, 129), 0.3, _ref_single("clustered", 129, 0.3), dets=d8[:, :6])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _candidates():
    """2 images x 2 classes, 300 rows: clustered boxes, a prediction tensor [2, 150, 8] and the candidate rows the filter half of
    non_max_suppression makes of it (score = obj * class_conf in fp32, as the wrapper computes it)"""
    rng = np.random.default_rng(5)
    d = R.clustered(300, 20, 11)
    d = d[rng.permutation(300)]
    pred = np.zeros((2, 150, 8), np.float32)
    pred[..., :6] = d.reshape(2, 150, 6)
    pred[..., 6:] = rng.uniform(0.2, 1.0, (2, 150, 2)).astype(np.float32)
    return pred


def test_pipeline_batched_loop_and_numpy_agree(cuda_dev, ops, tiles):
    from rotate_yolov3_amd.utils.nms import nms
    conf, thr = 0.1, 0.3
    pred = _candidates()
    pt = torch.from_numpy(pred)
    class_conf, class_pred = pt[..., 6:].max(2)
    score = pt[..., 5] * class_conf
    ok = (score > conf).nonzero()
    img, row = ok[:, 0], ok[:, 1]
    cand = torch.cat((pt[img, row][:, :5], score[img, row].unsqueeze(1), class_conf[img, row].unsqueeze(1), class_pred[img, row].unsqueeze(1).float()), 1)
    assert 200 < len(cand) < 300
    direct = nms.nms_from_candidates(img.to(cuda_dev), cand.to(cuda_dev), 2, thr, nc=2, nms_style="MERGE")
    batched = nms.non_max_suppression_batched(pt.clone().to(cuda_dev), conf, thr, nms_style="MERGE")
    loop = nms.non_max_suppression(pt.clone().to(cuda_dev), conf, thr, nms_style="MERGE")
    plain = nms.non_max_suppression(pt.clone().to(cuda_dev), conf, thr)
    want, bnd = R.pipeline(img.numpy(), cand.numpy(), 2, thr, 2)
    differs = 0
    for b in range(2):
        assert direct[b] is not None and want[b] is not None
        assert torch.equal(direct[b], batched[b]) and torch.equal(direct[b], loop[b])          # row for row, bit for bit
        got = direct[b].cpu().numpy()
        assert got.shape == want[b].shape
        assert np.array_equal(got[:, 5:].astype(np.float64), want[b][:, 5:])
        w32 = want[b][:, :5].astype(np.float32).astype(np.float64)
        assert (np.abs(got[:, :5].astype(np.float64) - w32) <= bnd[b]).all()
        # against 'OR': the same rows survive -- count, scores, class confidences, classes -- only the boxes move
        p = plain[b].cpu().numpy()
        assert p.shape == got.shape and np.array_equal(p[:, 5:], got[:, 5:])
        differs += int((p[:, :5] != got[:, :5]).any(1).sum())
    assert differs > 10


def test_darknet_detect_hands_the_style_through(cuda_dev):
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.utils.nms.nms import non_max_suppression_batched
    from tests.procedural import fill_procedural
    mg = fill_procedural(Darknet(make_cfg.tiny(), {"context_factor": 1.0}).eval()).to(cuda_dev)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(cuda_dev)
    with torch.no_grad():
        io, _ = mg(x)
        score = io[..., 5] * io[..., 6:].max(2)[0]
        thr = float(score.flatten().kthvalue(int(score.numel() * 0.5)).values)
        want = non_max_suppression_batched(io.clone(), thr, 0.3, nms_style="MERGE")
        plain = non_max_suppression_batched(io.clone(), thr, 0.3)
        got = mg.detect(x, thr, 0.3, nms_style="MERGE")
    assert [a is None for a in want] == [b is None for b in got] and any(a is not None for a in want)
    for a, b, p in zip(want, got, plain):
        if a is not None:
            assert torch.equal(a, b)
            assert torch.equal(a[:, 5:], p[:, 5:])
    with pytest.raises(ValueError):
        mg.detect(x, thr, 0.3, nms_style="SOFT")
