"""GPU tier: ryolo_det_rescale and ryolo_det_quads (csrc/detpost.hip) against their numpy restatements (tests/detect_reference.py)."""
import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.utils.detect_images import rescale_geometry
from tests import detect_reference as ref

pytestmark = pytest.mark.gpu

S = 96
GEOMETRY = [(1536, 2048), (97, 400), (64, 64)]      # (h0, w0)


def rows(m, seed):
    rng = np.random.default_rng(seed)
    det = rng.uniform(0, S, (m, 8)).astype(np.float32)
    det[:, 4] = rng.uniform(-1.5, 1.5, m)
    det[:, 5:] = rng.uniform(0, 1, (m, 3))
    return det


def run_rescale(det, det_off, geom, dev):
    d = torch.from_numpy(det.copy()).to(dev)
    got = ops.det_rescale(d, torch.tensor(det_off, dtype=torch.int32, device=dev), torch.from_numpy(geom).to(dev))
    assert got.data_ptr() == d.data_ptr()
    torch.cuda.synchronize(dev)
    return d.cpu().numpy()


@pytest.mark.parametrize("m", [0, 1, 300])
def test_rescale_one_image(cuda_dev, m):
    for k, shape in enumerate(GEOMETRY):
        det, geom = rows(m, 10 + k), rescale_geometry([shape], S)
        got = run_rescale(det, [0, m], geom, cuda_dev)
        want = ref.rescale(det, [0, m], geom)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shape
        assert np.array_equal(got[:, 4:].view(np.uint32), det[:, 4:].view(np.uint32))
        if m:
            assert not np.array_equal(got[:, :4], det[:, :4])


@pytest.mark.parametrize("m", [0, 1, 300])
def test_rescale_three_images_one_without_rows(cuda_dev, m):
    det, geom = rows(m, 20), rescale_geometry(GEOMETRY, S)
    for det_off in ([0, m // 3, m // 3, m], [0, 0, m - m // 4, m]):
        got = run_rescale(det, det_off, geom, cuda_dev)
        want = ref.rescale(det, det_off, geom)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), det_off
        assert np.array_equal(got[:, 4:].view(np.uint32), det[:, 4:].view(np.uint32))


def test_rescale_wrapper_refuses_other_layouts(cuda_dev):
    det = torch.zeros(4, 8, device=cuda_dev)
    off = torch.tensor([0, 4], dtype=torch.int32, device=cuda_dev)
    geom = torch.ones(1, 3, device=cuda_dev)
    with pytest.raises(RuntimeError, match="det must"):
        ops.det_rescale(det[:, :7], off, geom)
    with pytest.raises(RuntimeError, match="det_off"):
        ops.det_rescale(det, off.long(), geom)
    with pytest.raises(RuntimeError, match="geom"):
        ops.det_rescale(det, off, torch.ones(2, 3, device=cuda_dev))
    with pytest.raises(RuntimeError, match="det must"):
        ops.det_quads(det.double())


def test_quads_equal_the_float64_restatement(cuda_dev):
    det = ref.quad_boxes()
    keep = ref.comparable(det)
    print("det_quads: %d of %d boxes compared" % (keep.sum(), len(det)))
    assert keep.sum() >= 0.9 * len(det) and keep[:10].all()
    want, _ = ref.quads(det)
    before = det.copy()
    d = torch.from_numpy(det).to(cuda_dev)
    out = torch.full((len(det), 8), -(1 << 30), dtype=torch.int32, device=cuda_dev)
    got = ops.det_quads(d, out=out)
    torch.cuda.synchronize(cuda_dev)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(d.cpu().numpy(), before)
    got = got.cpu().numpy().astype(np.int64)
    assert (got != -(1 << 30)).all()
    assert np.array_equal(got[keep], want[keep]), np.argwhere((got != want).any(1) & keep)[:5]


def test_quads_of_no_rows_and_of_one(cuda_dev):
    assert tuple(ops.det_quads(torch.zeros(0, 8, device=cuda_dev)).shape) == (0, 8)
    det = np.array([[10, 20, 7, 3, 0, 0.9, 1, 0]], dtype=np.float32)
    got = ops.det_quads(torch.from_numpy(det).to(cuda_dev)).cpu().numpy()
    assert got.tolist() == [[6, 18, 13, 18, 13, 21, 6, 21]]


def test_side_stream_and_graph_replay(cuda_dev):
    det = ref.quad_boxes(seed=5, n=64)
    geom = rescale_geometry(GEOMETRY, S)
    det_off = [0, 20, 20, 64]
    src = rows(64, 3)
    want_r = ref.rescale(src, det_off, geom)
    d = torch.from_numpy(det).to(cuda_dev)
    want_q = ops.det_quads(d).cpu().numpy()
    r = torch.from_numpy(src.copy()).to(cuda_dev)
    off_t, geom_t = torch.tensor(det_off, dtype=torch.int32, device=cuda_dev), torch.from_numpy(geom).to(cuda_dev)
    q = torch.zeros(64, 8, dtype=torch.int32, device=cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    s = torch.cuda.Stream(cuda_dev)
    with torch.cuda.stream(s):
        ops.det_rescale(r, off_t, geom_t)
        ops.det_quads(d, out=q)
    s.synchronize()
    assert np.array_equal(r.cpu().numpy().view(np.uint32), want_r.view(np.uint32)) and np.array_equal(q.cpu().numpy(), want_q)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        ops.det_rescale(r, off_t, geom_t)
        ops.det_quads(d, out=q)
    for _ in range(2):
        r.copy_(torch.from_numpy(src))
        q.zero_()
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        assert np.array_equal(r.cpu().numpy().view(np.uint32), want_r.view(np.uint32)) and np.array_equal(q.cpu().numpy(), want_q)
