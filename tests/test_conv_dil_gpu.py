"""GPU tier of the matrix cfgs: ryolo_conv2d_dilated (csrc/conv_dil.hip) against fp32 ATen on the CPU, its slice / reproducibility /
batch properties, and the matrix model on the HIP engine against the bf16 emulation (tests/matrix_reference.py) and the reference's
fp32 golden.

Kernel tolerance: the project's conv tolerance (tests/test_conv_gpu.py), 2^-7 * |magnitude| + 2e-3, twice the relative part with a
residual (two roundings); inputs ~ N(0,1), weights ~ N(0,1) / sqrt(9 C_in), so outputs are O(1)."""
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
from tests import matrix_reference as mr
from tests.procedural import fill_procedural
from tests.test_matrix_cpu import bf16_emulation_error_vs_golden
from tests.test_model_gpu import _cmp

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
torch.set_num_threads(oracle.host_cores(16))

REL = 2.0 ** -7      # 2 bf16 ulp
ABS = 2e-3
BAR = (0.015, 0.0025)      # the project's engine-vs-emulation bar: max rel, mean rel (tests/test_model_gpu.py)


def _run(dev, n, h, w, cin, cout, dil, seed, residual=False, leaky=None, affine=False):
    x, wt = mr.conv_inputs(n, h, w, cin, cout, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    scale = torch.rand(cout, generator=g) + 0.5 if affine else torch.ones(cout)
    shift = torch.randn(cout, generator=g) * 0.5 if affine else torch.zeros(cout)
    res = torch.randn(n, h, w, cout, generator=g).to(torch.bfloat16) if residual else None
    want, mag = mr.dilated_reference(x, wt, dil, scale, shift, leaky, res)
    packed = ops.pack_weights(wt.to(dev), cin_pad=cin)
    sc, sh = ops.pad_vec(scale.to(dev), ops.cpad(cout)), ops.pad_vec(shift.to(dev), ops.cpad(cout))
    y = ops.conv2d_dilated(x.to(dev), packed, sc, sh, cout, dil, act=ops.ACT_LEAKY if leaky is not None else ops.ACT_LINEAR,
                           slope=leaky if leaky is not None else 0.0, residual=res.to(dev) if residual else None)
    torch.cuda.synchronize()
    err = (y.float().cpu() - want.float()).abs()
    tol = (2.0 if residual else 1.0) * REL * mag + ABS
    print("N %d %dx%d %d->%d dil %s: max err %.4g, mean |y| %.3g" % (n, h, w, cin, cout, dil, err.max().item(), want.float().abs().mean().item()))
    assert float(want.float().abs().mean()) > 0.2                   # O(1) outputs: the absolute floor is not what passes the test
    assert bool((err <= tol).all()), "max err %.4g (tol %.4g) at %s" % (
        err.max().item(), tol.flatten()[err.argmax()].item(), np.unravel_index(err.argmax().item(), err.shape))
    return y


@pytest.mark.parametrize("dil", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (1, 4), (8, 1)], ids=lambda d: "d%dx%d" % d)
def test_dilated_kernel_vs_aten_odd_map_two_images(cuda_dev, dil):
    """9 x 7 maps, M = 126 below any tile; (8,1) leaves only the centre row valid; two images, so a row test on the flat offset would read
    image 0 for the taps above row 0 of image 1"""
    _run(cuda_dev, 2, 9, 7, 64, 64, dil, seed=dil[0] * 10 + dil[1])


def test_dilated_kernel_undilated_equals_the_library_conv(cuda_dev):
    """dilation (1,1) is the plain 3x3: the same packed image through ryolo_conv2d_bn_act gives the same bits (same K order, same epilogue)"""
    x, wt = mr.conv_inputs(2, 9, 7, 64, 64, seed=5)
    packed = ops.pack_weights(wt.to(cuda_dev), cin_pad=64)
    sc, sh = torch.ones(128, device=cuda_dev), torch.zeros(128, device=cuda_dev)
    a = ops.conv2d_dilated(x.to(cuda_dev), packed, sc, sh, 64, (1, 1))
    b = ops.conv2d_bn_act(x.to(cuda_dev), packed, sc, sh, 64, 3, stride=1, pad=1, act=ops.ACT_LINEAR)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_dilated_kernel_residual_more_than_one_block(cuda_dev):
    _run(cuda_dev, 3, 12, 12, 128, 256, (1, 2), seed=1, residual=True)
    _run(cuda_dev, 3, 12, 12, 128, 256, (4, 1), seed=2, residual=True)


def test_dilated_kernel_long_k(cuda_dev):
    _run(cuda_dev, 1, 6, 6, 512, 128, (2, 1), seed=3)          # 72 K steps


def test_dilated_kernel_channel_count_that_fills_no_tile(cuda_dev):
    _run(cuda_dev, 2, 5, 11, 64, 40, (1, 2), seed=4)


def test_dilated_kernel_leaky_with_scale_and_shift(cuda_dev):
    _run(cuda_dev, 2, 9, 7, 64, 64, (2, 1), seed=6, leaky=0.1, affine=True)
    _run(cuda_dev, 2, 9, 7, 64, 64, (1, 2), seed=7, leaky=0.1, affine=True, residual=True)


def test_dilated_kernel_large_tile_path(cuda_dev):
    """enough 128 x 128 tiles for every CU (the threshold of the tile choice): 8 x 64 x 72 pixels x 128 channels = 288 tiles; an odd tail
    (M = 36864 + a partial row of tiles is covered by the 9 x 7 cases)"""
    _run(cuda_dev, 8, 64, 72, 64, 128, (1, 4), seed=8, residual=True)


def test_dilated_kernel_slices_keep_their_neighbours(cuda_dev):
    n, h, w, cin, cout, dil = 2, 9, 7, 64, 40, (1, 2)
    x, wt = mr.conv_inputs(n, h, w, cin, cout, seed=9)
    res = torch.randn(n, h, w, cout, generator=torch.Generator().manual_seed(10)).to(torch.bfloat16)
    want, mag = mr.dilated_reference(x, wt, dil, residual=res)
    xbuf = torch.full((n, h, w, 128), 7.0, dtype=torch.bfloat16, device=cuda_dev)
    xbuf[..., 24:88] = x.to(cuda_dev)
    ybuf = torch.full((n, h, w, 64), -3.0, dtype=torch.bfloat16, device=cuda_dev)
    rbuf = torch.full((n, h, w, 56), 5.0, dtype=torch.bfloat16, device=cuda_dev)
    rbuf[..., 8:48] = res.to(cuda_dev)
    packed = ops.pack_weights(wt.to(cuda_dev), cin_pad=cin)
    sc, sh = torch.ones(128, device=cuda_dev), torch.zeros(128, device=cuda_dev)
    ops.conv2d_dilated(xbuf[..., 24:88], packed, sc, sh, cout, dil, residual=rbuf[..., 8:48], out=ybuf[..., 16:56])
    torch.cuda.synchronize()
    err = (ybuf[..., 16:56].float().cpu() - want.float()).abs()
    assert bool((err <= 2.0 * REL * mag + ABS).all()), err.max().item()
    raw = ybuf.cpu().view(torch.int16)
    sentinel = torch.tensor([-3.0], dtype=torch.bfloat16).view(torch.int16).item()
    assert bool((raw[..., :16] == sentinel).all()) and bool((raw[..., 56:] == sentinel).all())
    assert bool((xbuf[..., :24] == 7.0).all()) and bool((xbuf[..., 88:] == 7.0).all()) and torch.equal(xbuf[..., 24:88].cpu(), x)
    assert bool((rbuf[..., :8] == 5.0).all()) and bool((rbuf[..., 48:] == 5.0).all()) and torch.equal(rbuf[..., 8:48].cpu(), res)


def test_dilated_kernel_is_bit_reproducible_and_batch_independent(cuda_dev):
    x, wt = mr.conv_inputs(2, 12, 12, 128, 256, seed=11)
    packed = ops.pack_weights(wt.to(cuda_dev), cin_pad=128)
    sc, sh = torch.ones(256, device=cuda_dev), torch.zeros(256, device=cuda_dev)
    xd = x.to(cuda_dev)
    a = ops.conv2d_dilated(xd, packed, sc, sh, 256, (2, 1))
    b = ops.conv2d_dilated(xd, packed, sc, sh, 256, (2, 1))
    one = ops.conv2d_dilated(xd[1:2].contiguous(), packed, sc, sh, 256, (2, 1))
    torch.cuda.synchronize()
    assert torch.equal(a, b)                      # two runs
    assert torch.equal(a[1:2], one)               # image 1 of a batch of 2 == the same image alone


# ---------------------------------------------------------------------------------------------------- the model
def _matrix_model(size, dev, na=8):
    cfg = make_cfg.darknet53_matrix(size, size, na_per_head=na)
    m = mr.fill_matrix(fill_procedural(Darknet(cfg, {"context_factor": 1.0}).eval()))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return cfg, sd, m.to(dev)


def _rel(a, b):
    scale = b.abs().mean().item() + 1e-6
    err = (a - b).abs()
    return (err / (b.abs() + scale)).max().item(), err.mean().item() / scale


def _bars(cfg, sd, x):
    """the bf16 emulation (io, p) and, per head and for io, the bar: the larger of the project's bar and twice the distance between the
    emulation accumulating its convs in fp32 and in fp64 -- both computed on the CPU, never from the engine's output"""
    io_e, p_e = mr.forward(cfg, sd, x, bf16=True)
    io_d, p_d = mr.forward(cfg, sd, x, bf16=True, acc64=True)
    bars = []
    for a, b in list(zip(p_e, p_d)) + [(io_e, io_d)]:
        d_max, d_mean = _rel(a, b)
        bars.append((max(BAR[0], 2 * d_max), max(BAR[1], 2 * d_mean), d_max, d_mean))
    return io_e, p_e, bars


@pytest.fixture(scope="module")
def model96(cuda_dev):
    """the 96^2 model, the golden's input, the bf16 emulation's result and the per-head bars: computed once, read by several tests"""
    cfg, sd, mg = _matrix_model(96, cuda_dev)
    x = torch.from_numpy(np.load(os.path.join(G, "forward_matrix_96.npz"))["x"])
    io_e, p_e, bars = _bars(cfg, sd, x)
    return cfg, sd, mg, x, io_e, p_e, bars


def _cmp_heads(tag, io, p, io_e, p_e, bars):
    for k in range(len(p_e)):
        print("%s p%d: fp32-vs-fp64 accumulation distance of the emulation: max rel %.4g  mean rel %.4g" % (tag, k, bars[k][2], bars[k][3]))
        _cmp("%s p%d" % (tag, k), p[k], p_e[k], rel_max=bars[k][0], rel_mean=bars[k][1])
    _cmp("%s io" % tag, io, io_e, rel_max=bars[-1][0], rel_mean=bars[-1][1])


def test_matrix_model_engine_vs_emulation_96(cuda_dev, model96):
    """Per head and for io: the project's bar (max rel 0.015, mean rel 0.0025) or, where the CPU shows the head to be more sensitive, twice
    the distance between the emulation accumulating in fp32 and in fp64 (_bars).  Measured (distance -> engine against the emulation, max
    rel / mean rel): FPN p0..p2 and the stride-64 p3: distance 0.0038..0.0072 / 0.0013..0.0019 -> engine 0.0038..0.0062 / 0.0012..0.0020
    (the project's bar holds); level 74 (3^2) p4 0.111 / 0.058 -> 0.038 / 0.027, p5 0.129 / 0.046 -> 0.052 / 0.035; level 86 (6^2)
    p6..p9 0.025..0.032 / 0.009..0.011 -> 0.018..0.026 / 0.008..0.010; level 98 (12^2) p10..p15 0.014..0.027 / 0.0045..0.0054 ->
    0.017..0.024 / 0.0045..0.0055; io 0.043 / 0.0057.  The matrix heads inherit the sensitivity of the trunk's feature maps (see
    tests/matrix_reference.py); every dilated launch by itself is held to the conv tolerance by the per-launch test below."""
    cfg, sd, mg, x, io_e, p_e, bars = model96
    with torch.no_grad():
        io, p = mg(x.to(cuda_dev))
    info = list(mg._engines.values())[0].op_info
    assert sum(i["name"].startswith("conv_dil<") for i in info) == 36 and len(p) == 16
    _cmp_heads("matrix", io, p, io_e, p_e, bars)


def test_matrix_model_every_dilated_launch_vs_aten_on_its_own_input(cuda_dev, model96):
    """The model-level bars of the matrix heads are loose (the heads are sensitive, see _bars and tests/test_matrix_cpu.py), so every one of
    the 36 dilated launches of the engine is also checked by itself: its input, residual and output views are read back after a forward and
    the output is compared with the CPU contract (mr.dilated_reference) on that very input and the source layer's weight.  Tolerance: the
    relative part of the conv tolerance (2^-7 of what gets rounded, twice with a residual) plus, in place of the absolute floor 2e-3 --
    it would be a tenth of the smaller of these tensors -- the worst-case difference of two fp32 summation orders, 2 K 2^-24 sum |w| |x|
    with K = 9 C_in.  Measured: max error 0 .. 0.0078 at mean |y| 0.13 .. 0.73."""
    cfg, sd, mg, x, io_e, p_e, bars = model96
    eng = HipEngine(mg, x.shape, cuda_dev)
    with torch.no_grad():
        eng(x.to(cuda_dev))
    torch.cuda.synchronize()
    defs, seen = mg.module_defs, 0
    for i, d in enumerate(defs):
        if d["type"] != "d-convolutional":
            continue
        dil = tuple(int(t) for t in d["dilation"].strip("()").split(","))
        w = sd["module_list.%d.Conv2d.weight" % int(d["weight_from"])]
        xin = eng.views[i - 1].cpu()
        folded = defs[i + 1]["type"] == "shortcut"
        res = eng.views[i - 2].cpu() if folded else None
        want, mag = mr.dilated_reference(xin, w, dil, residual=res)
        k = 9 * xin.shape[-1]
        order = torch.nn.functional.conv2d(xin.float().abs().permute(0, 3, 1, 2), w.to(torch.bfloat16).float().abs(), padding=dil,
                                           dilation=dil).permute(0, 2, 3, 1) * (2.0 * k * 2.0 ** -24)
        err = (eng.views[i].float().cpu() - want.float()).abs()
        tol = (2.0 if folded else 1.0) * REL * mag + order
        print("layer %d dil %s%s: mean |y| %.3g, max err %.3g" % (i, dil, " +res" if folded else "", want.float().abs().mean().item(), err.max().item()))
        assert bool((err <= tol).all()), (i, err.max().item(), tol.flatten()[err.argmax()].item())
        seen += 1
    assert seen == 36


def test_matrix_model_engine_vs_reference_golden(cuda_dev, model96):
    """against the reference's own fp32 output: the bar is 2 x the error the bf16 emulation itself has against that golden (computed here
    on the CPU), the rule of test_se_model_engine_vs_reference_golden.  Measured: emulation max rel 0.168 / mean rel 0.0194, engine 0.155 /
    0.0190."""
    cfg, sd, mg, x, io_e, p_e, bars = model96
    e_max, e_mean = bf16_emulation_error_vs_golden()
    print("bf16 emulation vs golden: max rel %.4g  mean rel %.4g" % (e_max, e_mean))
    z = np.load(os.path.join(G, "forward_matrix_96.npz"))
    with torch.no_grad():
        io, p = mg(x.to(cuda_dev))
    _cmp("matrix io vs fp32 reference", io, torch.from_numpy(z["io"]), rel_max=2 * e_max, rel_mean=2 * e_mean)


def test_matrix_model_graph_replay_equals_eager(cuda_dev, model96):
    cfg, sd, mg, x, io_e, p_e, bars = model96
    xg = x.to(cuda_dev)
    eager = HipEngine(mg, xg.shape, cuda_dev)
    io0, p0 = eager(xg)
    io0, p0 = io0.clone(), [q.clone() for q in p0]
    graphed = HipEngine(mg, xg.shape, cuda_dev, use_graph=True)
    for _ in range(2):                                    # capture, then a second replay
        io1, p1 = graphed(xg)
        torch.cuda.synchronize()
        assert torch.equal(io0, io1) and all(torch.equal(a, b) for a, b in zip(p0, p1))


def test_matrix_model_aliasing_changes_no_bit(cuda_dev, model96, monkeypatch):
    """the nine aliased shared layers: launching them again instead (RYOLO_SHARED_ALIAS=0) gives the same bits"""
    cfg, sd, mg, x, io_e, p_e, bars = model96
    xg = x.to(cuda_dev)
    a = HipEngine(mg, xg.shape, cuda_dev)
    monkeypatch.setenv("RYOLO_SHARED_ALIAS", "0")
    b = HipEngine(mg, xg.shape, cuda_dev)
    assert len(b.ops) == len(a.ops) + 9
    io0, p0 = a(xg)
    io1, p1 = b(xg)
    torch.cuda.synchronize()
    assert torch.equal(io0, io1) and all(torch.equal(u, v) for u, v in zip(p0, p1))


def test_matrix_model_detect_equals_forward_plus_nms(cuda_dev):
    from rotate_yolov3_amd.utils.nms.nms import non_max_suppression
    cfg, sd, mg = _matrix_model(160, cuda_dev)
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


def test_matrix_source_weight_update_is_noticed(cuda_dev):
    """negating layer 100's weight in place (the first 3x3 of the 12^2 level, read by its own launch and by six dilated sharers): the next
    forward rebuilds the engine, the six matrix heads of that level change, and the result is the emulation's on the new state dict"""
    cfg, sd, mg = _matrix_model(96, cuda_dev)
    x = torch.rand(1, 3, 96, 96, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        io0, p0 = mg(x.to(cuda_dev))
        mg.module_list[100].Conv2d.weight.mul_(-1.0)
        io1, p1 = mg(x.to(cuda_dev))
    assert all(not torch.equal(p0[k], p1[k]) for k in range(10, 16))
    assert all(torch.equal(p0[k], p1[k]) for k in (0, 1, 3, 4, 5, 6, 7, 8, 9))           # the other levels read other weights
    sd2 = {k: v.cpu() for k, v in mg.state_dict().items()}
    assert torch.equal(sd2["module_list.100.Conv2d.weight"], -sd["module_list.100.Conv2d.weight"])
    io_e, p_e, bars = _bars(cfg, sd2, x)
    _cmp_heads("matrix after the update", io1, p1, io_e, p_e, bars)


def test_matrix_training_is_refused_on_the_hip_path_and_runs_on_torch(cuda_dev):
    cfg, sd, mg = _matrix_model(96, cuda_dev)
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    mg.train()
    with pytest.raises(plan.Refused, match="backend = 'torch'"):
        mg(x)
    mg.backend = "torch"
    p = mg(x)
    assert len(p) == len(mg.yolo_layers) == 16 and p[4].shape == (2, 8, 3, 3, 7)
    assert all(q.requires_grad and bool(torch.isfinite(q).all()) for q in p)
