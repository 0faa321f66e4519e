"""GPU tier: an NHWC8Batch (model/nhwc_batch.py: a batch already in the engines' bf16 [N, H, W, 8] input layout) handed to Darknet.forward,
the eval engine and the TrainEngine gives the bits of the fp32 NCHW tensor it was made from, without the converter pass."""
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.model.nhwc_batch import NHWC8Batch
from rotate_yolov3_amd.utils.synthetic import synthetic_targets
from tests.test_train_engine_gpu import HYP, _run, _well_conditioned

pytestmark = pytest.mark.gpu
S, BS = 64, 2


def same_bits(a, b):
    """bit for bit, NaN included (an untrained eval model decodes some boxes to inf / NaN, which torch.equal never calls equal)"""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    differ = int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())
    print("%s: %d of %d values differ in their bits, %d NaN" % (tuple(a.shape), differ, a.numel(), int(torch.isnan(a).sum())))
    return differ == 0


@pytest.fixture(scope="module")
def setup(cuda_dev):
    m = _well_conditioned(Darknet(make_cfg.darknet53(S, S), dict(HYP))).to(cuda_dev)
    m.nc, m.arc = 1, "default"
    x32 = torch.rand(BS, 3, S, S, generator=torch.Generator().manual_seed(7)).to(cuda_dev)
    return m, x32, NHWC8Batch(ops.nchw_f32_to_nhwc_bf16(x32))


def test_the_batch_object(cuda_dev, setup):
    _, x32, batch = setup
    assert tuple(batch.shape) == (BS, 3, S, S) and len(batch) == BS and batch.is_cuda and batch.device == x32.device
    assert batch.to(cuda_dev) is batch and batch.to("cuda") is batch
    back = batch.float()                                  # ryolo_nhwc_bf16_to_nchw_f32: the fp32 tensor after the engines' own rounding
    assert back.dtype == torch.float32 and torch.equal(back, x32.to(torch.bfloat16).float())
    assert not batch.data[..., 3:].any()
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.to("cpu")
    with pytest.raises(TypeError):                        # only the device can change: a dtype or a flag is not quietly dropped
        batch.to(cuda_dev, dtype=torch.float16)
    with pytest.raises(TypeError):
        batch.to(cuda_dev, non_blocking=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        NHWC8Batch(torch.zeros((1, S, S, 8), dtype=torch.bfloat16))
    for bad in (torch.zeros((1, S, S, 8), device=cuda_dev), torch.zeros((1, S, S, 16), dtype=torch.bfloat16, device=cuda_dev),
                torch.zeros((1, S, 8, S), dtype=torch.bfloat16, device=cuda_dev).permute(0, 1, 3, 2)):
        with pytest.raises(ValueError):
            NHWC8Batch(bad)


def test_copy_into_copies_unless_the_batch_is_the_buffer(cuda_dev, setup):
    _, _, batch = setup
    buf = torch.full((BS, S, S, 8), 3.0, dtype=torch.bfloat16, device=cuda_dev)
    assert batch.copy_into(buf) is True and torch.equal(buf.view(torch.int16), batch.data.view(torch.int16))
    assert NHWC8Batch(buf).copy_into(buf) is False          # the same memory: nothing is enqueued
    assert NHWC8Batch(buf.clone()).copy_into(buf) is True   # equal values elsewhere are still copied
    wide = torch.zeros((BS, S, S, 16), dtype=torch.bfloat16, device=cuda_dev)
    view = wide[..., :8]                                     # an input buffer that is a channel slice of a wider one
    assert batch.copy_into(view) is True and torch.equal(view.contiguous().view(torch.int16), batch.data.view(torch.int16))
    assert not wide[..., 8:].any()
    for other in (torch.zeros((BS + 1, S, S, 8), dtype=torch.bfloat16, device=cuda_dev),
                  torch.zeros((BS, S, S + 32, 8), dtype=torch.bfloat16, device=cuda_dev)):
        with pytest.raises(RuntimeError, match="planned for"):
            batch.copy_into(other)


def test_eval_heads_are_bit_identical_and_the_converter_is_skipped(cuda_dev, setup):
    m, x32, batch = setup
    m.eval()
    m.backend = 'hip'
    with torch.no_grad():
        io_b, p_b = m(x32)
        with _lib.trace_calls() as log:
            io_a, p_a = m(batch)
    assert same_bits(io_a, io_b) and len(p_a) == len(p_b) == 3 and all(same_bits(a, b) for a, b in zip(p_a, p_b))
    names = [c[0] for c in log]
    assert names and "ryolo_nchw_f32_to_nhwc_bf16" not in names
    eng = m.engine(batch.shape, cuda_dev)
    assert eng.x_nhwc.is_contiguous() and eng.x_nhwc.data_ptr() != batch.data.data_ptr()
    own = NHWC8Batch(eng.x_nhwc)                          # the engine's own input buffer handed back: not even a copy
    assert own.copy_into(eng.x_nhwc) is False and batch.copy_into(eng.x_nhwc) is True
    with torch.no_grad():
        io_c, _ = m(own)
    assert same_bits(io_c, io_a)
    det_a, det_b = m.detect(batch, 0.3, 0.5), m.detect(x32, 0.3, 0.5)
    assert len(det_a) == len(det_b) == BS
    for a, b in zip(det_a, det_b):
        assert (a is None) == (b is None) and (a is None or same_bits(a, b))
    other = NHWC8Batch(torch.zeros((BS + 1, S, S, 8), dtype=torch.bfloat16, device=cuda_dev))
    with pytest.raises(RuntimeError, match="planned for"):     # a batch of another size goes to its own engine, never into this one's buffer
        eng(other)


def test_the_graph_engine_replays_the_layers_behind_the_copy(cuda_dev, setup):
    """use_graph=True: an NHWC8Batch is copied into the input buffer in front of a graph of the layers alone -- no conversion back to
    fp32, no converter inside the graph -- and the fp32 path's own graph is not disturbed by it"""
    from rotate_yolov3_amd.model.engine import HipEngine
    m, x32, batch = setup
    m.eval()
    m.backend = 'hip'
    with torch.no_grad():
        io_e, p_e = m(x32)
        eng = HipEngine(m, batch.shape, cuda_dev, use_graph=True)
        io_1 = eng(batch)[0].clone()                      # warm-up + capture + replay
        other = NHWC8Batch(ops.nchw_f32_to_nhwc_bf16(1.0 - x32))
        io_o = eng(other)[0].clone()                      # a replay on other data
        with _lib.trace_calls() as log:
            io_2, p_2 = eng(batch)                        # a replay: no library call at all, the copy is torch's
        assert [c[0] for c in log] == [] and eng.graph is None and eng.graph_layers is not None
        assert same_bits(io_1, io_e) and same_bits(io_2, io_e) and all(same_bits(a, b) for a, b in zip(p_2, p_e))
        assert not same_bits(io_o, io_e)
        io_f = eng(x32)[0].clone()                        # the fp32 graph beside it
        assert eng.graph is not None and same_bits(io_f, io_e) and same_bits(eng(batch)[0], io_e)


def test_the_aten_chain_receives_the_fp32_tensor(cuda_dev, setup, monkeypatch):
    """backend 'torch' converts the batch with ryolo_nhwc_bf16_to_nchw_f32 before the operator chain.  The tensor the chain is handed
    is compared, not what it computes: the chain's convolutions are not bit-reproducible from call to call."""
    m, x32, batch = setup
    seen = []
    real = m._torch_forward
    monkeypatch.setattr(m, "_torch_forward", lambda x: (seen.append(x), real(x))[1])
    m.eval()
    m.backend = 'torch'
    try:
        with torch.no_grad():
            io_t, p_t = m(batch)
    finally:
        m.backend = 'hip'
    assert len(seen) == 1 and torch.is_tensor(seen[0]) and same_bits(seen[0], x32.to(torch.bfloat16).float())
    assert tuple(io_t.shape) == (BS, 6048, 7) and len(p_t) == 3


def test_training_heads_are_bit_identical(cuda_dev, setup):
    m, x32, batch = setup
    m.backend = 'hip'
    m.train()
    tg = synthetic_targets(BS, seed=5, device=cuda_dev)
    # whole steps (forward, loss, backward): two eager ones, the capture, two replays -- the hand-over sits in front of the graph
    runs = [_run(m, x, tg) for x in (x32, batch, batch, x32, batch)]
    m.eval()
    p0, l0, g0 = runs[0]
    assert len(p0) == 3
    for p, l, g in runs[1:]:
        assert l == l0 and all(torch.equal(a, b) for a, b in zip(p, p0)) and all(torch.equal(g[k], g0[k]) for k in g0)
    other = NHWC8Batch(torch.zeros((BS + 1, S, S, 8), dtype=torch.bfloat16, device=cuda_dev))
    with pytest.raises(RuntimeError, match="planned for"):
        m.train_engine((BS, 3, S, S), cuda_dev).forward(other)
