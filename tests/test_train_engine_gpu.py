"""GPU tier: one training step (forward with batch-stat BN + hand-written backward) of Darknet-53 on the HIP TrainEngine
vs the ATen fp32 autograd chain (the reference's operator chain) on the same weights, input and targets."""
import copy

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model.loss import compute_loss
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.utils.synthetic import synthetic_targets
from tests.procedural import fill_procedural

pytestmark = pytest.mark.gpu
HYP = {"giou": 0.1, "cls": 27.76, "cls_pw": 1.0, "obj": 20.35, "obj_pw": 1.0, "iou_t": 0.5, "ang_t": 3.1415926 / 12,
       "reg": 1.0, "fl_gamma": 0.5, "context_factor": 1.0}


def _well_conditioned(model, seed=5):
    """variance-preserving random conv weights, non-trivial BN affine: unlike the procedural sin() weights these do not
    turn the 75 batch-stat BatchNorm layers into a noise amplifier, so run-to-run atomics-order noise stays small"""
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        for name, t in model.state_dict().items():
            if t.dim() == 4:
                t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * (6.0 / t[0].numel()) ** 0.5)
            elif name.endswith("BatchNorm2d.weight"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("BatchNorm2d.bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
    return model


def _run(model, x, targets, autocast=False):
    model.zero_grad(set_to_none=True)
    if autocast:     # the bf16 contract of the HIP engine: bf16 conv in/out, fp32 accumulation and BatchNorm math
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            pred = model(x)
    else:
        pred = model(x)
    loss, items = compute_loss([p.float() for p in pred], targets.clone(), model, model.hyp)
    loss.backward()
    return [p.detach().float().cpu() for p in pred], float(loss.detach()), {k: v.grad.detach().float().cpu().clone()
                                                                            for k, v in model.named_parameters() if v.grad is not None}


def test_train_step_matches_aten_autograd(cuda_dev):
    size, bs = 160, 4
    cfg = make_cfg.darknet53(size, size)
    torch.manual_seed(0)
    ref = Darknet(cfg, dict(HYP))
    _well_conditioned(ref)
    ref = ref.to(cuda_dev).train()
    ref.nc, ref.arc = 1, "default"
    ref.backend = "torch"
    hip = copy.deepcopy(ref)
    hip.backend = "hip"
    hip._engines = {}
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(0)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=3, device=cuda_dev)
    # Three runs on identical weights: fp32 ATen (ground truth), bf16-autocast ATen (PyTorch's own bf16 contract, the
    # yardstick) and the HIP engine.  bf16 noise grows through 75 batch-stat BatchNorm layers, so the bar is RELATIVE:
    # the engine must sit as close to fp32 as PyTorch's bf16 path does.
    ref32 = copy.deepcopy(ref)
    p_f, loss_f, g_f = _run(ref32, x, tg)
    p_r, loss_r, g_r = _run(ref, x, tg, autocast=True)
    p_h, loss_h, g_h = _run(hip, x, tg)

    def rel(a, b):
        return (a - b).abs().mean().item() / (b.abs().mean().item() + 1e-12)
    for k in range(3):
        e_h, e_r = rel(p_h[k], p_f[k]), rel(p_r[k], p_f[k])
        print("head %d: mean rel err vs fp32: hip %.4f  autocast %.4f" % (k, e_h, e_r))
        assert e_h <= 1.3 * e_r + 0.01
    print("loss fp32 %.5f  autocast %.5f  hip %.5f" % (loss_f, loss_r, loss_h))
    assert abs(loss_h - loss_f) <= 1.5 * abs(loss_r - loss_f) + 0.02 * abs(loss_f)
    assert set(g_h) == set(g_f)

    def cosines(g, gf):
        dots = na = nb = 0.0
        per = {}
        for k in gf:
            a, b = g[k].flatten().double(), gf[k].flatten().double()
            dots += float(a @ b); na += float(a @ a); nb += float(b @ b)
            per[k] = float(a @ b / (a.norm() * b.norm() + 1e-30))
        return dots / (na ** 0.5 * nb ** 0.5 + 1e-30), (na / nb) ** 0.5, per
    c_h, n_h, per_h = cosines(g_h, g_f)
    c_r, n_r, per_r = cosines(g_r, g_f)
    print("gradient vs fp32: hip cos %.5f norm ratio %.4f | autocast cos %.5f norm ratio %.4f" % (c_h, n_h, c_r, n_r))
    worse = [(k, round(per_h[k], 3), round(per_r[k], 3)) for k in per_h if per_h[k] < per_r[k] - 0.1]
    print("tensors where hip is >0.1 below autocast in cosine: %d of %d" % (len(worse), len(per_h)), worse[:10])
    assert c_h >= c_r - 0.03 and abs(n_h - 1.0) <= abs(n_r - 1.0) + 0.1
    # noise-dominated tensors (deep PReLU slopes, BN shifts) flip either way from run to run (atomic order): 12-17 seen
    assert len(worse) <= 0.08 * len(per_h)
    # BatchNorm running statistics were updated like nn.BatchNorm2d does
    bn_h, bn_r = hip.module_list[1][1], ref32.module_list[1][1]
    assert torch.allclose(bn_h.running_mean, bn_r.running_mean, rtol=2e-2, atol=2e-3)
    assert torch.allclose(bn_h.running_var, bn_r.running_var, rtol=2e-2, atol=2e-3)
    assert int(bn_h.num_batches_tracked) == 1


def test_second_step_accumulates_and_reuses_buffers(cuda_dev):
    size, bs = 128, 4
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=4, device=cuda_dev)
    _, l1, g1 = _run(m, x, tg)
    pred = m(x)                                     # second backward WITHOUT zero_grad: gradients add up
    loss, _ = compute_loss([p.float() for p in pred], tg.clone(), m, m.hyp)
    loss.backward()
    # BN statistics are batch statistics and the step is bit-reproducible (fp64 statistic atomics, fixed-order split-K and slab
    # reductions: DESIGN 3.4), so the second pass adds EXACTLY the first pass's gradient: every tensor is 2 x the single-step one
    named = dict(m.named_parameters())
    for k, a in g1.items():
        g2 = named[k].grad.float().cpu()
        assert torch.equal(g2, a + a), (k, float((g2 - 2 * a).abs().max()), float(a.abs().max()))
    # third / fourth step go through the captured hipGraphs: same bits as the eager steps
    for _ in range(2):
        _, l3, g3 = _run(m, x, tg)
        assert l3 == l1
        for k in g1:
            assert torch.equal(g3[k], g1[k]), (k, float((g3[k] - g1[k]).abs().max()))


def test_training_step_is_bit_reproducible(cuda_dev):
    """loss, heads and all parameter gradients of a step are identical from run to run -- eager steps, hipGraph
    replays, and a FRESH engine on a copy of the model (different buffer addresses, different atomic arrival orders)."""
    size, bs = 160, 4
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    m2 = copy.deepcopy(m)
    m2._engines = {}
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(2)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=5, device=cuda_dev)
    runs = [_run(m, x, tg) for _ in range(5)]          # 2 eager steps, capture, 2 replays
    runs.append(_run(m2, x, tg))
    p0, l0, g0 = runs[0]
    for r, (p, l, g) in enumerate(runs[1:], 1):
        assert l == l0, (r, l, l0)
        for a, b in zip(p, p0):
            assert torch.equal(a, b), (r, float((a - b).abs().max()))
        for k in g0:
            assert torch.equal(g[k], g0[k]), (r, k, float((g[k] - g0[k]).abs().max()), float(g0[k].abs().max()))


@pytest.mark.parametrize("impl,riou,arc", [("hip", 0, "default"), ("torch", 0, "default"), ("hip", 1, "default"),
                                           ("hip", 0, "Fdefault"), ("hip", 0, "uBCE"), ("hip", 0, "FuCE")])
def test_fused_loss_graph_equals_eager_mirror(cuda_dev, impl, riou, arc):
    """Darknet.enable_fused_loss(): compute_loss on the engine's heads is one hipGraph replay of the fixed-shape
    formulation.  On the SAME head tensors it must give the eager mirror's loss items and head gradients; steps 0-1 run
    it eagerly, step 2 captures, step 3 replays -- with different targets every step (count and content).
    riou = 1: the rotated-IoU loss (hyp['riou']; eager = autograd through RotatedIoU, fused = iou_mode 1 of the loss kernel).
    arc: the focal / unified arcs of the reference (loss.py:284-286, :350-360) stay on the HIP kernels too."""
    size, bs = 128, 4
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP, riou=riou))).to(cuda_dev).train()
    assert m.hyp.get("riou", 0) == riou
    m.nc, m.arc = 1, arc
    m.enable_fused_loss(capacity=32, impl=impl)
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    for step in range(5):
        tg = synthetic_targets(bs if step != 3 else 2, seed=20 + step, device=cuda_dev)
        if step == 4:
            tg = tg[:0]                                   # no targets at all
        pred = m(x)
        pl = [p.detach().clone().float().requires_grad_(True) for p in pred]
        fused, m.fused_loss = m.fused_loss, None
        loss_ref, items_ref = compute_loss(pl, tg.clone(), m, m.hyp)
        loss_ref.backward()
        m.fused_loss = fused
        loss, items = compute_loss([p.float() for p in pred], tg.clone(), m, m.hyp)
        eng = [e for e in m._engines.values() if hasattr(e, "_fused_state")][0]
        assert torch.allclose(items, items_ref, rtol=1e-4, atol=1e-6), (step, items, items_ref)
        if impl == "hip":
            # the NHWC loss kernel writes d loss / d head straight into the head conv's bf16 gradient buffers (the fp32
            # buffers stay all-zero scratch): compare those, at bf16 resolution, in the layout the backward consumes
            assert eng.fused_nhwc and all(float(b.abs().max()) == 0.0 for b in eng.static_pg)
            for (_, hg), q in zip(eng.head_pairs, pl):
                want = q.grad.permute(0, 2, 3, 1, 4).reshape(hg.shape)
                assert torch.allclose(hg.float(), want, rtol=2 ** -7, atol=1e-9), (step, (hg.float() - want).abs().max())
        else:
            for g, q in zip(eng.static_pg, pl):
                assert torch.allclose(g, q.grad, rtol=2e-3, atol=1e-8), (step, (g - q.grad).abs().max())
        loss.backward()                                   # the engine's backward consumes the fused head gradients
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        m.zero_grad(set_to_none=True)
    assert eng._fused_state['graph'] is not None


def test_fused_loss_refuses_stale_or_repeated_backward(cuda_dev):
    """the fused loss writes d loss / d head into engine buffers at loss time -- backward of an OLDER loss (another
    compute_loss ran since) or a second backward through the same loss would silently use the wrong gradient: both raise."""
    size, bs = 128, 2
    m = _well_conditioned(Darknet(make_cfg.darknet53(size, size), dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    m.enable_fused_loss(capacity=32)
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=21, device=cuda_dev)
    pred = m(x)
    loss_a, _ = compute_loss([p.float() for p in pred], tg.clone(), m, m.hyp)
    loss_b, _ = compute_loss([p.float() for p in pred], tg.clone(), m, m.hyp)
    with pytest.raises(RuntimeError, match="overwritten by a later"):
        loss_a.backward()
    loss_b.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        loss_b.backward()


def test_bn_reduce_folded_into_the_dgrad_at_608_geometry(cuda_dev, monkeypatch):
    """At the batch / geometry of configs[3] the reduce pass of a 3x3 block's BatchNorm backward runs inside the 1x1 data gradient
    that produces its dy (needs tile lists the small test shapes do not have: bs 16 at 608^2 engages it at 76^2 and above).
    The folded step is bit-reproducible (eager steps, graph replays) and agrees with the separate-pass engine up to the summation
    order of the per-channel sums."""
    size, bs = 608, 16
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    m2 = copy.deepcopy(m)
    m2._engines = {}
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=6, device=cuda_dev)
    monkeypatch.setenv("RYOLO_BN_REDUCE_FUSION", "1")
    runs = [_run(m, x, tg, autocast=True) for _ in range(4)]
    eng = [e for e in m._engines.values() if hasattr(e, "bplan")][0]
    folded = [pl for kind, i, pl, f in eng.bplan if kind == 'conv' and pl.red_for is not None]
    assert len(folded) >= 8, len(folded)
    p0, l0, g0 = runs[0]
    for p, l, g in runs[1:]:
        assert l == l0
        for k in g0:
            assert torch.equal(g[k], g0[k]), k
    monkeypatch.setenv("RYOLO_BN_REDUCE_FUSION", "0")
    p1, l1, g1 = _run(m2, x, tg, autocast=True)
    eng2 = [e for e in m2._engines.values() if hasattr(e, "bplan")][0]
    assert not any(pl.red_for is not None for kind, i, pl, f in eng2.bplan if kind == 'conv')
    assert l1 == l0                                             # the forward is untouched
    # the per-channel sums are added in another order (rows per workgroup instead of pixel slabs): dz moves by a bf16 ulp in a few
    # elements, and that noise reaches the parameter gradients in proportion to their conditioning.  Tensors: cosine / norm;
    # the PReLU slope gradients are single scalars, each a sum over a whole layer with heavy cancellation: judged as one vector
    sa, sb = [], []
    for k in g0:
        a, b = g0[k].double().flatten(), g1[k].double().flatten()
        if a.numel() == 1:
            sa.append(a)
            sb.append(b)
            continue
        if float(b.norm()) == 0.0:
            assert float(a.norm()) == 0.0, k
            continue
        cos = float(a @ b / (a.norm() * b.norm()))
        assert cos > 0.998 and abs(float(a.norm() / b.norm()) - 1.0) < 0.04, (k, cos, float(a.norm() / b.norm()))   # (norm bar of the composed-backward test)
    sa, sb = torch.cat(sa), torch.cat(sb)
    assert float(sa @ sb / (sa.norm() * sb.norm())) > 0.995
    assert bool(((sa - sb).abs() <= 0.35 * torch.maximum(sa.abs(), sb.abs()) + 0.02 * sb.abs().max()).all()), (sa - sb).abs().max()
    del m, m2
    torch.cuda.empty_cache()


def test_configs3_bs64_608_step_equals_the_bs4_step_on_a_16_times_repeated_batch(cuda_dev):
    """BASELINE configs[3] at its own size: one train step with the riou loss at bs 64, 608^2, through the product path (Darknet.forward ->
    TrainEngine, loss mirror, engine backward).  The batch is four images x 16 with the targets repeated per copy, so that -- the loss being a
    mean over cells / targets and BatchNorm statistics of a repeated batch being those of the four images -- heads, loss and EVERY parameter
    gradient must equal the bs-4 step's.  What differs is everything batch-dependent in the dispatch (wide-tile choice, persistent-grid depth,
    folded BatchNorm reduces, split-K counts) and the order of the statistics sums, i.e. bf16-rounding noise, which 75 batch-statistics
    BatchNorm layers amplify: the bars are RELATIVE to a yardstick, the ATen chain under bf16 autocast on the same four images (first GPU run of
    this test: head 0 differs by 6.6 % mean-relative between the bs-4 and the bs-64 evaluation).  Inside the bs-64 batch every copy of an image
    has bit-identical heads."""
    import ctypes
    from rotate_yolov3_amd import _lib
    from rotate_yolov3_amd.model import hip_ops as ops
    size = 608
    cfg = make_cfg.darknet53(size, size)
    hyp = dict(HYP)
    hyp["riou"] = 1
    m4 = _well_conditioned(Darknet(cfg, hyp)).to(cuda_dev).train()
    m4.nc, m4.arc = 1, "default"
    m64 = copy.deepcopy(m4)
    m64._engines = {}
    ref = copy.deepcopy(m4)              # (before m4 runs: its engine holds ctypes records, which do not deep-copy)
    ref._engines = {}
    ref.backend = "torch"
    x4 = torch.rand(4, 3, size, size, generator=torch.Generator().manual_seed(11)).to(cuda_dev)
    tg4 = synthetic_targets(4, seed=12, device=cuda_dev)
    x64 = x4.repeat(16, 1, 1, 1)
    tg64 = torch.cat([tg4 + torch.tensor([4.0 * r, 0, 0, 0, 0, 0, 0], device=cuda_dev) for r in range(16)])
    p4, l4, g4 = _run(m4, x4, tg4)
    p64, l64, g64 = _run(m64, x64, tg64)
    # the yardstick (as in test_train_step_matches_aten_autograd): PyTorch's own bf16 contract -- the ATen chain under autocast -- on the
    # SAME four images.  bf16 rounding noise grows through 75 batch-statistics BatchNorm layers, so "equal" means: the bs-64 step sits as
    # close to the bs-4 HIP step as another legitimate bf16 evaluation of that bs-4 step does.
    p_r, l_r, g_r = _run(ref, x4, tg4, autocast=True)

    def rel(a, b):
        return (a - b).abs().mean().item() / (b.abs().mean().item() + 1e-12)
    for k in range(3):
        for i in range(4, 64):
            assert torch.equal(p64[k][i], p64[k][i % 4]), (k, i)
        e64, e_r = rel(p64[k][:4], p4[k]), rel(p_r[k], p4[k])
        print("head %d vs the bs-4 HIP step, mean rel err: bs-64 copy %.5f | ATen autocast bs 4 %.5f" % (k, e64, e_r))
        assert e64 <= 1.3 * e_r + 0.01, (k, e64, e_r)
    print("loss: bs 4 %.6f  bs 64 %.6f  ATen autocast bs 4 %.6f" % (l4, l64, l_r))
    assert abs(l64 - l4) <= 1.5 * abs(l_r - l4) + 0.01 * abs(l4), (l4, l64, l_r)
    assert set(g64) == set(g4)

    def cosines(g, gf):
        dots = na = nb = 0.0
        per = {}
        for k in gf:
            a, b = g[k].flatten().double(), gf[k].flatten().double()
            dots += float(a @ b); na += float(a @ a); nb += float(b @ b)
            per[k] = float(a @ b / (a.norm() * b.norm() + 1e-30))
        return dots / (na ** 0.5 * nb ** 0.5 + 1e-30), (na / nb) ** 0.5, per
    c64, n64, per64 = cosines(g64, g4)
    c_r, n_r, per_r = cosines(g_r, g4)
    print("gradients vs the bs-4 HIP step: bs 64 cos %.5f norm ratio %.4f | ATen autocast cos %.5f norm ratio %.4f" % (c64, n64, c_r, n_r))
    # (single-element tensors -- the 72 PReLU slopes, each a sum over a whole layer with heavy cancellation -- have cosine +-1: they are judged
    # as ONE vector below, as in the folded-reduce test)
    worse = [(k, round(per64[k], 3), round(per_r[k], 3)) for k in per64 if g4[k].numel() > 1 and per64[k] < per_r[k] - 0.1]
    print("tensors where bs 64 is > 0.1 below the yardstick in cosine: %d of %d" % (len(worse), len(per64)), worse[:10])
    assert c64 >= c_r - 0.03 and abs(n64 - 1.0) <= abs(n_r - 1.0) + 0.1
    assert len(worse) <= 0.05 * len(per64)
    sk = [k for k in g4 if g4[k].numel() == 1]
    s64, s4, s_r = [torch.cat([g[k].flatten().double() for k in sk]) for g in (g64, g4, g_r)]
    cs64, cs_r = float(s64 @ s4 / (s64.norm() * s4.norm())), float(s_r @ s4 / (s_r.norm() * s4.norm()))
    print("PReLU slope gradients as one vector (%d entries): bs 64 vs bs 4 cosine %.5f | ATen autocast vs bs 4 %.5f" % (len(sk), cs64, cs_r))
    # (first GPU run: 0.35 vs 0.17 -- at this size, with random weights, the slope gradients are dominated by the bf16 noise of either evaluation)
    assert cs64 >= cs_r - 0.05
    del ref
    # the batch-dependent dispatch at bs 64: wide tiles on conv_mq, folded BatchNorm reduces, the 128-channel family
    eng = [e for e in m64._engines.values() if hasattr(e, "bplan")][0]
    folded = [pl for kind, i, pl, f in eng.bplan if kind == 'conv' and pl.red_for is not None]
    assert len(folded) >= 40, len(folded)
    L = _lib.lib()
    fwd, dgr = {}, {}
    for blk in eng.blocks:
        d = blk.desc
        key = "k%d s%d %d->%d @%d" % (blk.k, blk.s, blk.conv.in_channels, blk.C, blk.y.shape[1])
        fwd[key] = ops.kernel_name_of(L.ryolo_conv_kernel_choice(ctypes.byref(d), 0, 1 if blk.bn is not None else 0), blk.k, blk.s, d.Cin)
        if blk.xin_g is not None:
            dgr[key] = ops.kernel_name_of(L.ryolo_conv_dgrad_kernel_choice(ctypes.byref(d), 1 if blk.red_for is not None else 0), blk.k, 1, d.Cout)
    print("bs-64 forward kernels:", sorted(set(fwd.values())))
    print("bs-64 data-gradient kernels:", sorted(set(dgr.values())))
    assert fwd["k3 s1 128->256 @76"] == 'conv_mq<k3,128x256>' and fwd["k3 s1 256->512 @38"] == 'conv_mq<k3,128x256>'
    assert dgr["k3 s1 256->512 @38"] == 'conv_mq<k3,128x256>'
    assert fwd["k3 s1 64->128 @152"] == 'conv3x3_c64_halo' and fwd["k3 s2 64->128 @152"].startswith('conv_igemm<k3,128x128'), fwd
    assert dgr["k3 s1 128->256 @76"] == 'conv_igemm<k3,128x128>', dgr
    del m4, m64
    torch.cuda.empty_cache()


def test_reducer_buckets_fire_during_segmented_backward(cuda_dev):
    """With a GradientAllReducer attached (one-rank RCCL group on this GPU) the engine cuts its backward at the bucket
    boundaries, flushes each segment's gradients into the bucket views and runs the reducer's hooks: every bucket's
    all-reduce is in flight before finish().  Gradients equal the unsegmented engine's up to its run-to-run noise."""
    import os
    import torch.distributed as dist
    from rotate_yolov3_amd.dist import GradientAllReducer
    size, bs = 128, 4
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=4, device=cuda_dev)
    _, l0, g0 = _run(m, x, tg)                                   # plain engine, one segment
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    try:
        m.refresh_engines()
        dp = GradientAllReducer(m, bucket_mb=32.0)
        assert len(dp.buckets) >= 4
        for step in range(4):                                     # eager, eager, capture, replay
            pred = m(x)
            loss, _ = compute_loss([p.float() for p in pred], tg.clone(), m, m.hyp)
            loss.backward()
            assert all(b["handle"] is not None for b in dp.buckets), "a bucket's all-reduce was not launched by the hooks"
            dp.finish()
            g = {k: v.grad.detach().float().cpu().clone() for k, v in m.named_parameters()}
            dp.zero_grad()
        eng = [e for e in m._engines.values() if hasattr(e, "_segs")][0]
        assert len(eng._segs) >= 4 and all(gr is not None for gr in eng.g_bwd)
        for k in g0:      # segmented backward + one-rank all-reduce: the same bits as the unsegmented pass
            assert torch.equal(g[k], g0[k]), (k, float((g[k] - g0[k]).abs().max()), float(g0[k].abs().max()))
        # with the reducer attached the kernels accumulate straight into the bucket views (no second buffer, no add pass) ...
        assert eng.direct and eng.static_flat is None
        assert all(eng.static_grad[q].data_ptr() == q.grad.data_ptr() for q in m.parameters())
        # ... and when the user replaces param.grad (zero_grad(set_to_none=True)) the engine puts the bucket views back: the reducer's
        # hooks all-reduce the BUCKETS, so a gradient anywhere else would be stepped on un-averaged.  Same gradients.
        import warnings
        for _ in range(3):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, l1, g1 = _run(m, x, tg)                        # zero_grad(set_to_none=True) inside
            assert eng.direct and eng.static_flat is None
            assert all(eng.static_grad[q].data_ptr() == q.grad.data_ptr() for q in m.parameters())
            assert l1 == l0
            for k in g0:
                assert torch.equal(g1[k], g0[k]), k
            dp.finish()
    finally:
        dist.destroy_process_group()


def test_eval_after_training_step_sees_the_updated_weights(cuda_dev):
    """the eval engine packs weights / folds BatchNorm at construction and is cached per shape; after a training
    step (parameters and running statistics changed) an eval forward must not reuse the stale copy."""
    from rotate_yolov3_amd.utils.fused_sgd import FusedSGD
    torch.manual_seed(1)
    m = _well_conditioned(Darknet(make_cfg.darknet53(64, 64), dict(HYP))).to(cuda_dev)
    m.nc, m.arc = 1, "default"
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(cuda_dev)
    tg = synthetic_targets(4, seed=4, device=cuda_dev)
    m.eval()
    with torch.no_grad():
        io0 = m(x)[1][0].clone()                   # builds and caches the eval engine (raw head 0: the decode's exp overflows on random weights)
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, nesterov=True)
    m.train()
    for _ in range(3):
        opt.zero_grad(set_to_none=False)
        loss, _ = compute_loss([p.float() for p in m(x)], tg.clone(), m, m.hyp)
        loss.backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        io1 = m(x)[1][0].clone()
        m.backend = "torch"
        want = m(x)[1][0]
        m.backend = "hip"
    assert (io1 - io0).abs().max().item() > 1e-3, "the training steps changed nothing?"
    err = (io1 - want).abs().mean().item() / want.abs().mean().item()
    assert err < 0.02, "eval after training differs from the ATen chain on the same weights: %.4f" % err


def test_eval_engines_follow_optimizer_steps_and_manual_edits(cuda_dev):
    """the staleness of the cached eval engines follows the PARAMETER UPDATE, not the training forward: train-forward,
    backward, eval (engines rebuilt), optimizer.step(), eval -- the second eval must see the stepped weights; so must an eval
    after an in-place edit with no training forward at all (EMA, manual surgery)."""
    from rotate_yolov3_amd.utils.fused_sgd import FusedSGD
    torch.manual_seed(2)
    m = _well_conditioned(Darknet(make_cfg.darknet53(64, 64), dict(HYP))).to(cuda_dev)
    m.nc, m.arc = 1, "default"
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    tg = synthetic_targets(4, seed=5, device=cuda_dev)
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, nesterov=True)

    def eval_head():
        m.eval()
        with torch.no_grad():
            got = m(x)[1][0].clone()
            m.backend = "torch"
            want = m(x)[1][0]
            m.backend = "hip"
        return got, (got - want).abs().mean().item() / want.abs().mean().item()

    m.train()
    loss, _ = compute_loss([p.float() for p in m(x)], tg.clone(), m, m.hyp)
    loss.backward()
    h1, e1 = eval_head()                       # eval BETWEEN backward and step: rebuilds the engines from the old weights
    m.train()
    opt.step()                                 # no training forward follows
    h2, e2 = eval_head()
    assert e1 < 0.02 and e2 < 0.02, (e1, e2)
    assert (h2 - h1).abs().max().item() > 1e-4, "the optimizer step changed nothing?"
    with torch.no_grad():                      # manual in-place edit, no optimizer, no training forward
        m.module_list[0][0].weight.mul_(1.5)
    h3, e3 = eval_head()
    assert e3 < 0.02 and (h3 - h2).abs().max().item() > 1e-4, e3


def test_unsupported_activation_raises_instead_of_running_linear(cuda_dev):
    """Swish (eval + train) and Mish (train) used to be dropped silently on the HIP paths."""
    CFG = make_cfg.darknet53(64, 64)
    assert "activation=leaky" in CFG
    x = torch.rand(2, 3, 64, 64).to(cuda_dev)
    m = Darknet(CFG.replace("activation=leaky", "activation=swish", 1), dict(HYP)).to(cuda_dev).eval()
    with pytest.raises(RuntimeError, match="not on the HIP path"):
        m(x)
    m.backend = "torch"
    assert torch.isfinite(m(x)[0]).all()
    m2 = Darknet(CFG.replace("activation=leaky", "activation=swish", 1), dict(HYP)).to(cuda_dev).train()
    with pytest.raises(RuntimeError, match="no HIP training kernels"):
        m2(x)
    # Mish (the north star's activation) trains on the HIP path since r2 (bn_act kernels, act code 2)
    m3 = Darknet(CFG.replace("activation=leaky", "activation=mish"), dict(HYP)).to(cuda_dev).train()
    assert all(torch.isfinite(p).all() for p in m3(x))


MINI_CFG = """
[net]
width=128
height=128
channels=3

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=32
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-3
activation=linear

[convolutional]
batch_normalize=1
filters=128
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=128
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-3
activation=linear

[convolutional]
batch_normalize=1
filters=256
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=128
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=256
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-3
activation=linear

[convolutional]
size=1
stride=1
pad=1
filters=56
activation=linear

[yolo]
mask = 16-23
anchors = 20,6, 40,10, 80,20
classes=1
num=3

[route]
layers = -3

[convolutional]
batch_normalize=1
filters=64
size=1
stride=1
pad=1
activation=leaky

[upsample]
stride=2

[route]
layers = -1, 8

[convolutional]
batch_normalize=1
filters=128
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=56
activation=linear

[yolo]
mask = 8-15
anchors = 20,6, 40,10, 80,20
classes=1
num=3

[route]
layers = -3

[convolutional]
batch_normalize=1
filters=64
size=1
stride=1
pad=1
activation=leaky

[upsample]
stride=2

[route]
layers = -1, 4

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=56
activation=linear

[yolo]
mask = 0-7
anchors = 20,6, 40,10, 80,20
classes=1
num=3
"""


class _RoundBf16(torch.autograd.Function):
    """value and gradient both pass through a bf16 store, like the engine's activation / gradient buffers"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


@pytest.mark.parametrize("activation", ["leaky", "mish"])
def test_composed_backward_is_sharp_against_the_bf16_storage_contract(cuda_dev, activation):
    """the whole-step check on the 75-layer net is noise-bound (cos ~0.58, as bad as autocast).  This one is
    sharp: an fp32 ATen autograd chain that rounds to bf16 exactly where the engine STORES bf16 (conv output z, block output y,
    and the gradients flowing back through both), with bf16-representable weights and input -- what remains is accumulation
    order.  The composed plan (gradient-buffer sharing along residual chains, first-write-overwrites, concat slices, upsample,
    stride-2 parity classes in situ, three heads) must then reproduce EVERY parameter gradient.  Measured (r2): lowest per-tensor
    cosine 0.9919, norm ratios 0.98-1.005 -- what is left is the bf16 rounding of the engine's IN-PLACE gradient accumulation at
    shortcut fan-ins and of the folded scale/shift form of BatchNorm, which the hook emulation does not reproduce; the bar is
    cosine >= 0.985, norm +-4 % for every tensor (the old whole-net bar was 0.6).  This test found the head-bias reduction bug
    fixed in csrc/train.hip (channels >= 32 of a 56-channel head were never reduced: cosine 0.24).
    `mish`: the same network with every PReLU replaced by Mish (act code 2 of the bn_act kernels)."""
    torch.manual_seed(3)
    ref = Darknet(MINI_CFG.replace("activation=leaky", "activation=" + activation), dict(HYP))
    with torch.no_grad():
        g = torch.Generator().manual_seed(11)
        for name, t in ref.state_dict().items():
            if t.dim() == 4:
                t.copy_(((torch.rand(t.shape, generator=g) * 2 - 1) * (6.0 / t[0].numel()) ** 0.5).to(torch.bfloat16).float())
            elif name.endswith("BatchNorm2d.weight"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("BatchNorm2d.bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
    # the reference chain runs on the CPU (fp32 ATen, deterministic); on the GPU MIOpen's algorithm search and atomics made the
    # REFERENCE differ from run to run by more than the bar.  The HIP engine itself is bit-reproducible (fp64 statistics atomics,
    # fixed-order split-K and slab reductions; tools/determinism_check.py)
    ref = ref.train()
    ref.nc, ref.arc = 1, "default"
    hip = copy.deepcopy(ref).to(cuda_dev)
    ref.backend, hip.backend = "torch", "hip"
    hip._engines = {}
    # the bf16 storage points of the engine, as hooks on the ATen chain
    for mdef, mod in zip(ref.module_defs, ref.module_list):
        if mdef["type"] == "convolutional":
            mod[0].register_forward_hook(lambda m, i, o: _RoundBf16.apply(o))            # z
            if len(mod) > 1:
                mod.register_forward_hook(lambda m, i, o: _RoundBf16.apply(o))           # y = act(bn(z))
    bs = 8
    x = torch.rand(bs, 3, 128, 128, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).float().to(cuda_dev)
    tg = synthetic_targets(bs, seed=6, device=cuda_dev)
    p_r, loss_r, g_r = _run(ref, x.cpu(), tg.cpu())
    p_h, loss_h, g_h = _run(hip, x, tg)
    for k in range(3):
        e = (p_h[k] - p_r[k]).abs().mean().item() / p_r[k].abs().mean().item()
        print("head %d mean rel err vs the bf16-contract chain: %.5f" % (k, e))
        assert e < 1e-2, (k, e)
    assert abs(loss_h - loss_r) < 2e-3 * abs(loss_r), (loss_h, loss_r)
    assert set(g_h) == set(g_r)
    worst, scal = [], []
    for k in g_r:
        a, b = g_h[k].flatten().double(), g_r[k].flatten().double()
        if float(b.norm()) < 1e-12:
            continue
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        ratio = float(a.norm() / b.norm())
        if a.numel() == 1:
            # PReLU slopes: ONE number = sum over every negative pre-activation of dy * u, a heavily cancelling sum whose bf16
            # noise grows with the backward depth (the per-op test pins the kernel's dslope to 2e-3 on identical inputs; here the
            # deepest ones can even change sign against the fp32 chain) -- judged together below, on the scale of the largest
            scal.append((float(a), float(b), k))
            continue
        worst.append((cos, ratio, k))
    worst.sort()
    print("lowest cosines:", [(round(c, 5), round(r, 4), k) for c, r, k in worst[:5]])
    assert len(worst) > 40
    for cos, ratio, k in worst:
        assert cos >= 0.985 and abs(ratio - 1.0) <= 0.04, (k, cos, ratio)
    if scal:
        va, vb = torch.tensor([t[0] for t in scal]).double(), torch.tensor([t[1] for t in scal]).double()
        big = float(vb.abs().max())
        print("slope gradients (engine, chain):", [(round(x, 4), round(y, 4)) for x, y, _ in scal])
        assert float(va @ vb / (va.norm() * vb.norm())) >= 0.95 and float((va - vb).abs().max()) <= 0.15 * big, scal


def test_failed_graph_capture_falls_back_to_eager_launches(cuda_dev, monkeypatch):
    """a runtime that refuses stream capture (e.g. under a multi-rank RCCL group) must cost speed, not the run.
    torch.cuda.graph is made to fail from the third step on; the engine and the fused loss continue with eager launches, say so in
    `graph_fallback`, and produce the bits of the captured run."""
    size, bs = 128, 4
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    m2 = copy.deepcopy(m)
    m2._engines = {}
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=6, device=cuda_dev)
    ref = [_run(m, x, tg) for _ in range(4)][-1]                  # eager, eager, capture, replay

    class Refuse(object):
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            raise RuntimeError("HIP error: operation not permitted when stream is capturing (simulated)")

        def __exit__(self, *a):
            return False

    monkeypatch.setattr(torch.cuda, "graph", Refuse)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = [_run(m2, x, tg) for _ in range(4)][-1]
    eng = [e for e in m2._engines.values() if hasattr(e, "_segs")][0]
    assert eng.use_graph is False and eng.graph_fallback and "simulated" in eng.graph_fallback
    assert got[1] == ref[1]
    for k in ref[2]:
        assert torch.equal(got[2][k], ref[2][k]), k


def test_no_graph_switch_runs_the_same_kernels_eagerly(cuda_dev, monkeypatch):
    """RYOLO_NO_GRAPH=1 (bench.py --no-graph, the fallback a launcher can use when a runtime refuses stream capture under a multi-rank
    communicator): engine and fused HIP loss launch eagerly from the first step -- the same kernels, the same bits as the graph-replayed
    steps, and NOT the eager ATen loss mirror."""
    size, bs = 128, 4
    cfg = make_cfg.darknet53(size, size)
    hyp = dict(HYP)
    hyp["riou"] = 1
    m = _well_conditioned(Darknet(cfg, hyp)).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    m2 = copy.deepcopy(m)
    m2._engines = {}
    m.enable_fused_loss(capacity=256)
    m2.enable_fused_loss(capacity=256)
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=6, device=cuda_dev)
    ref = [_run(m, x, tg) for _ in range(4)][-1]                  # eager, eager, capture, replay
    monkeypatch.setenv("RYOLO_NO_GRAPH", "1")
    got = [_run(m2, x, tg) for _ in range(4)][-1]
    eng = [e for e in m2._engines.values() if hasattr(e, "_segs")][0]
    assert eng.use_graph is False and eng.no_graph_env and eng.g_fwd is None and eng.graph_fallback is None
    st = eng._fused_state                                         # the fused loss ran (its state lives on the engine), without a graph
    assert st['calls'] == 4 and st['graph'] is None
    # the REPORTED loss of the fused HIP loss is summed with one fp32 atomic per workgroup (csrc/loss.hip: the dense kernels' `items`),
    # so its last bit depends on arrival order (seen once: 1.3160331 vs 1.3160332); nothing in the step reads it -- the gradients below
    # are what the step computes, and they are compared bit for bit
    assert abs(got[1] - ref[1]) <= 4e-7 * abs(ref[1])
    for k in ref[2]:
        assert torch.equal(got[2][k], ref[2][k]), k


def test_batched_split_k_reduce_gives_the_bits_of_the_per_layer_reduces(cuda_dev, monkeypatch):
    """TrainEngine with the segment-wide reduce launch (round 5 default: every conv's partial tiles in its own workspace, ONE
    ryolo_conv_wgrad_reduce_batch per backward segment) against RYOLO_WGRAD_BATCH_REDUCE=0 (one reduce behind every weight gradient):
    loss and every gradient bit for bit, eager steps and graph replays, with a reducer attached (four segments) and without."""
    from rotate_yolov3_amd.dist import GradientAllReducer
    size, bs = 128, 4
    cfg = make_cfg.darknet53(size, size)
    m = _well_conditioned(Darknet(cfg, dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    m2 = copy.deepcopy(m)
    m2._engines = {}
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    tg = synthetic_targets(bs, seed=6, device=cuda_dev)
    ref = [_run(m, x, tg) for _ in range(4)]                       # eager, eager, capture, replay
    eng = [e for e in m._engines.values() if hasattr(e, "_segs")][0]
    assert eng.batch_reduce and len(eng._wr_batches) == 1 and list(eng._wr_batches.values())[0].n >= 70
    monkeypatch.setenv("RYOLO_WGRAD_BATCH_REDUCE", "0")
    got = [_run(m2, x, tg) for _ in range(4)]
    eng2 = [e for e in m2._engines.values() if hasattr(e, "_segs")][0]
    assert not eng2.batch_reduce and not eng2._wr_batches
    for r, q in zip(ref, got):
        assert r[1] == q[1]
        for k in r[2]:
            assert torch.equal(r[2][k], q[2][k]), k


@pytest.mark.parametrize("case", ["all_trainable", "stem_weight_frozen", "per_layer_reduce"])
def test_the_launch_bodies_allocate_nothing_on_their_first_call(cuda_dev, monkeypatch, case):
    """_forward_launch and _backward_launch are what the hipGraphs capture: everything they need exists after __init__ and
    _prepare_backward().  torch's allocation counter (with the allocated and reserved bytes) must not move across the FIRST call of
    each, where a lazy allocation would have nowhere to hide.  Darknet-53 at 64^2, batch 2 (heads 2^2, 4^2, 8^2: the smallest input the
    engine accepts); a frozen stem weight takes layer 0's two-pass backward with its own workspace, RYOLO_WGRAD_BATCH_REDUCE=0 the
    shared split-K workspace."""
    size, bs = 64, 2
    if case == "per_layer_reduce":
        monkeypatch.setenv("RYOLO_WGRAD_BATCH_REDUCE", "0")
    m = _well_conditioned(Darknet(make_cfg.darknet53(size, size), dict(HYP))).to(cuda_dev).train()
    m.nc, m.arc = 1, "default"
    if case == "stem_weight_frozen":
        m.module_list[0].Conv2d.weight.requires_grad_(False)
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(7)).to(cuda_dev).contiguous()
    eng = m.train_engine(x.shape, cuda_dev)

    def allocator():
        return (torch.cuda.memory_stats(cuda_dev).get("allocation.all.allocated"), torch.cuda.memory_allocated(cuda_dev),
                torch.cuda.memory_reserved(cuda_dev))
    with torch.cuda.device(cuda_dev), torch.no_grad():
        eng.x_nhwc.zero_()
        eng.x_nhwc[..., :3].copy_(x.permute(0, 2, 3, 1))
        torch.cuda.synchronize(cuda_dev)
        before = allocator()
        eng._forward_launch()
        assert allocator() == before, ("forward", before, allocator())
        for _, hg in eng.head_pairs:
            hg.fill_(0.01)
        segs = eng._prepare_backward()
        assert eng._prepare_backward() is segs                     # idempotent
        for lo, hi, _ in segs:
            before = allocator()
            eng._backward_launch(lo, hi)
            assert allocator() == before, ("backward", lo, hi, before, allocator())
        torch.cuda.synchronize(cuda_dev)
    b0 = eng.blocks[0]
    assert before[0] is not None, "torch.cuda.memory_stats has no allocation counter on this build"
    assert b0.ws0 is not None and b0.one_pass == (case != "stem_weight_frozen") and (b0.dz is None) == b0.one_pass
    assert (eng._ws_w is not None) == (case == "per_layer_reduce") == (not eng.batch_reduce)
    assert all((b.ws_w is not None) == (eng.batch_reduce and b.has_wgrad) for b in eng.blocks)
    g = eng.static_grad[m.module_list[1].Conv2d.weight]
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
