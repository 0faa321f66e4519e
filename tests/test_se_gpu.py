"""GPU tier of the squeeze-and-excitation layers: ryolo_se_nhwc (csrc/se.hip) against fp64, its stride / reproducibility / batch
properties, and the se model on the HIP engine against the bf16 emulation (tests/se_reference.py) and the reference's fp32 golden.

Bars of the kernel tests: y within 1 bf16 ulp of bf16(x * g_fp64) and at most 0.5 % of the elements different at all (the gate's
relative error is of the order of fp32 epsilon, far below the bf16 half-ulp 2^-9: only values on a rounding boundary can move, by
one step; fp32 ATen on these inputs: max 1 ulp, < 0.01 % different); gate_out within max(1e-6, 8 x the error fp32 ATen makes on
the same inputs) of fp64 (the factor allows for another summation order and expf)."""
import os

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
import oracle
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model import plan
from rotate_yolov3_amd.model.engine import HipEngine
from rotate_yolov3_amd.model.models import Darknet
from tests import se_reference as sr
from tests.procedural import fill_procedural
from tests.test_model_gpu import _cmp
from tests.test_se_cpu import bf16_emulation_error_vs_golden

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
torch.set_num_threads(oracle.host_cores(16))

SHAPES = [(2, 8, 8, 256), (3, 5, 7, 512), (2, 2, 2, 1024), (1, 19, 19, 1024), (2, 13, 9, 64), (1, 1, 1, 16), (2, 6, 6, 40),
          (2, 76, 76, 256)]


def _check(y, gate, x, w1, w2, tag):
    """the Numerics bars against fp64 on the same bf16 inputs and fp32 weights"""
    y64, g64 = sr.se_fp64(x, w1, w2)
    _, g32 = sr.se_aten_fp32(x, w1, w2)
    d = sr.bf16_ulp_diff(y.cpu(), y64.to(torch.bfloat16))
    frac = float((d > 0).double().mean())
    gerr = float((gate.cpu().double() - g64).abs().max())
    aten = float((g32.double() - g64).abs().max())
    bar = max(1e-6, 8 * aten)
    print("%s: y max %d ulp, %.4f %% differ; gate err %.3g (fp32 ATen %.3g, bar %.3g)" % (tag, int(d.max()), 100 * frac, gerr, aten, bar))
    assert int(d.max()) <= 1 and frac <= 0.005, (tag, int(d.max()), frac)
    assert gerr <= bar, (tag, gerr, bar)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_se_kernel_vs_fp64(cuda_dev, shape):
    n, h, w, c = shape
    x, w1, w2 = sr.unit_inputs(n, h, w, c, seed=c + h)
    gate = torch.full((n, c), -1.0, device=cuda_dev)
    y = ops.se_nhwc(x.to(cuda_dev), w1.to(cuda_dev), w2.to(cuda_dev), gate_out=gate)
    torch.cuda.synchronize()
    _check(y, gate, x, w1, w2, "se %s" % (shape,))


def test_se_kernel_strided_views_keep_their_neighbours(cuda_dev):
    n, h, w, c = 2, 7, 9, 256
    x, w1, w2 = sr.unit_inputs(n, h, w, c, seed=11)
    xbuf = torch.full((n, h, w, 384), 7.0, dtype=torch.bfloat16, device=cuda_dev)
    xbuf[..., 64:320] = x.to(cuda_dev)
    ybuf = torch.full((n, h, w, 272), -3.0, dtype=torch.bfloat16, device=cuda_dev)
    gate = torch.empty((n, c), device=cuda_dev)
    ops.se_nhwc(xbuf[..., 64:320], w1.to(cuda_dev), w2.to(cuda_dev), out=ybuf[..., 8:264], gate_out=gate)
    torch.cuda.synchronize()
    _check(ybuf[..., 8:264].contiguous(), gate, x, w1, w2, "strided")
    raw = ybuf.cpu().view(torch.int16)
    sentinel = torch.tensor([-3.0], dtype=torch.bfloat16).view(torch.int16).item()
    assert bool((raw[..., :8] == sentinel).all()) and bool((raw[..., 264:] == sentinel).all())
    assert bool((xbuf[..., :64] == 7.0).all()) and bool((xbuf[..., 320:] == 7.0).all()) and torch.equal(xbuf[..., 64:320].cpu(), x)
    # two disjoint slices of ONE buffer are accepted, an overlapping pair is refused
    both = torch.zeros((n, h, w, 512), dtype=torch.bfloat16, device=cuda_dev)
    both[..., :256] = x.to(cuda_dev)
    ops.se_nhwc(both[..., :256], w1.to(cuda_dev), w2.to(cuda_dev), out=both[..., 256:])
    torch.cuda.synchronize()
    assert torch.equal(both[..., 256:].cpu(), ybuf[..., 8:264].cpu())
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.se_nhwc(both[..., :256], w1.to(cuda_dev), w2.to(cuda_dev), out=both[..., 128:384])


@pytest.mark.parametrize("shape", [(2, 76, 76, 256), (1, 19, 19, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_se_kernel_is_bit_reproducible(cuda_dev, shape):
    n, h, w, c = shape
    x, w1, w2 = (t.to(cuda_dev) for t in sr.unit_inputs(n, h, w, c, seed=3))
    outs = []
    for _ in range(2):
        gate = torch.empty((n, c), device=cuda_dev)
        outs.append((ops.se_nhwc(x, w1, w2, gate_out=gate), gate))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_se_kernel_batch_independence(cuda_dev):
    x, w1, w2 = (t.to(cuda_dev) for t in sr.unit_inputs(2, 8, 8, 256, seed=5))
    g2, g1 = torch.empty((2, 256), device=cuda_dev), torch.empty((1, 256), device=cuda_dev)
    y2 = ops.se_nhwc(x, w1, w2, gate_out=g2)
    y1 = ops.se_nhwc(x[1:2].contiguous(), w1, w2, gate_out=g1)
    torch.cuda.synchronize()
    assert torch.equal(y2[1:2], y1) and torch.equal(g2[1:2], g1)


# ---------------------------------------------------------------------------------------------------- the model
def _se_model(size, dev):
    cfg = make_cfg.darknet53_se(size, size)
    m = sr.fill_se(fill_procedural(Darknet(cfg, {"context_factor": 1.0}).eval()))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return cfg, sd, m.to(dev)


@pytest.fixture(scope="module")
def model64(cuda_dev):
    """the 64^2 model, its input and the bf16 emulation's result: computed once, read by several tests, never modified"""
    cfg, sd, mg = _se_model(64, cuda_dev)
    x = torch.from_numpy(np.load(os.path.join(G, "forward_d53se_64.npz"))["x"])
    io_e, p_e = sr.forward(cfg, sd, x, bf16=True)
    return cfg, sd, mg, x, io_e, p_e


def test_se_model_engine_vs_emulation_64(cuda_dev, model64):
    """The bars of the plain engine-vs-oracle tests (rel_max 0.015, rel_mean 0.0025).  Measured: p0 max rel 0.0049 / mean rel 0.0022,
    p1 0.0048 / 0.0015, p2 0.0039 / 0.0005, io 0.0038 / 0.0003.  p0 is close to its mean bar, and not because of the se kernels: layer
    by layer against the emulation the engine is within 0.02 % up to layer 11; the stride-2 conv 12 -- in front of the first se,
    identical in the plain cfg -- turns that into 0.35 % (its sums cancel: output scale 0.23 from an input of scale 1.6), the stride-2
    convs 45 and 78 into about 2 %, and each se layer hands on what it receives.  At 2 x 2 head cells this model amplifies last-bit
    differences: an earlier se_gate with another (equally exact) summation order gave p0 0.0077 / 0.0048, and accumulating the
    emulation's own convs in fp64 instead of fp32 moves its p0 by mean rel 0.0013 (0.0008 for the plain cfg)."""
    cfg, sd, mg, x, io_e, p_e = model64
    with torch.no_grad():
        io, p = mg(x.to(cuda_dev))
    assert sum(i["name"] == "se_nhwc" and i["flops"] == 0 for i in list(mg._engines.values())[0].op_info) == 20
    for k in range(3):
        _cmp("se p%d" % k, p[k], p_e[k], rel_max=0.015, rel_mean=0.0025)
    _cmp("se io", io, io_e, rel_max=0.015, rel_mean=0.0025)


def test_se_model_engine_vs_emulation_96_bs2(cuda_dev):
    cfg, sd, mg = _se_model(96, cuda_dev)                 # odd map sizes 12 / 6 / 3
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        io, p = mg(x.to(cuda_dev))
    io_e, p_e = sr.forward(cfg, sd, x, bf16=True)
    for k in range(3):
        _cmp("se96 p%d" % k, p[k], p_e[k], rel_max=0.015, rel_mean=0.0025)
    _cmp("se96 io", io, io_e, rel_max=0.015, rel_mean=0.0025)


def test_se_model_engine_vs_reference_golden(cuda_dev, model64):
    """against the reference's own fp32 output: the bar is 2 x the error the bf16 emulation itself has against that golden (computed
    here on the CPU; the factor 2 is the one test_model_gpu._cmp documents for the plain model)"""
    cfg, sd, mg, x, io_e, p_e = model64
    e_max, e_mean = bf16_emulation_error_vs_golden()
    print("bf16 emulation vs golden: max rel %.4g  mean rel %.4g" % (e_max, e_mean))
    z = np.load(os.path.join(G, "forward_d53se_64.npz"))
    with torch.no_grad():
        io, p = mg(x.to(cuda_dev))
    _cmp("se io vs fp32 reference", io, torch.from_numpy(z["io"]), rel_max=2 * e_max, rel_mean=2 * e_mean)


def test_se_model_graph_replay_equals_eager(cuda_dev, model64):
    cfg, sd, mg, x, io_e, p_e = model64
    xg = x.to(cuda_dev)
    eager = HipEngine(mg, xg.shape, cuda_dev)
    io0, p0 = eager(xg)
    io0, p0 = io0.clone(), [q.clone() for q in p0]
    graphed = HipEngine(mg, xg.shape, cuda_dev, use_graph=True)
    for _ in range(2):                                    # capture, then a second replay
        io1, p1 = graphed(xg)
        torch.cuda.synchronize()
        assert torch.equal(io0, io1) and all(torch.equal(a, b) for a, b in zip(p0, p1))


def test_se_model_detect_equals_forward_plus_nms(cuda_dev):
    from rotate_yolov3_amd.utils.nms.nms import non_max_suppression
    cfg, sd, mg = _se_model(160, cuda_dev)
    x = torch.rand(3, 3, 160, 160, generator=torch.Generator().manual_seed(5)).to(cuda_dev)
    with torch.no_grad():
        io, _ = mg(x)
    score = io[..., 5] * io[..., 6:].max(2)[0]
    thr = float(score.flatten().kthvalue(int(score.numel() * 0.97)).values)
    want = non_max_suppression(io.clone(), thr, 0.3)
    got = mg.detect(x, thr, 0.3)
    assert [a is None for a in want] == [b is None for b in got]
    for a, b in zip(want, got):
        if a is not None:
            assert torch.equal(a, b)
    assert sum(len(a) for a in want if a is not None) > 50


def test_se_weight_update_is_noticed(cuda_dev):
    cfg, sd, mg = _se_model(64, cuda_dev)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        io0, _ = mg(x.to(cuda_dev))
        mg.module_list[13].fc[2].weight.mul_(-1.0)        # in place: every gate of the first se moves to 1 - g
        io1, _ = mg(x.to(cuda_dev))
    assert not torch.equal(io0, io1)
    sd2 = {k: v.cpu() for k, v in mg.state_dict().items()}
    assert not torch.equal(sd2["module_list.13.fc.2.weight"], sd["module_list.13.fc.2.weight"])
    io_e, _ = sr.forward(cfg, sd2, x, bf16=True)
    _cmp("se io after the update", io1, io_e, rel_max=0.015, rel_mean=0.0025)


def test_se_training_is_refused_on_the_hip_path_and_runs_on_torch(cuda_dev):
    cfg, sd, mg = _se_model(64, cuda_dev)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    mg.train()
    with pytest.raises(plan.Refused, match="backend = 'torch'"):
        mg(x)
    mg.backend = "torch"
    p = mg(x)
    assert len(p) == 3 and p[0].shape == (2, 72, 2, 2, 7) and p[0].requires_grad and bool(torch.isfinite(p[0]).all())
