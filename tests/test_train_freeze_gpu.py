"""GPU tier: the HIP TrainEngine honours requires_grad (rotate-yolov3_amd/model/train_engine.py, model/plan.py `trainable`).

Darknet-53 at 64 x 64, batch 2, one class: the smallest shape that still has three heads (2^2, 4^2, 8^2), the residual chains, both
routes and the stem paths.  The reference for the bits is the all-trainable HIP engine on a deep copy of the same model with the same
input and targets -- the code path of before: a frozen step launches a subset of its kernels on the same operands with the same
split-K plan, so every gradient that is still computed must come out bit for bit (torch.equal), as must heads, loss and the BatchNorm
running statistics.

Patterns: A `--transfer` (weight and bias of the convs in front of the yolo layers, 81 / 93 / 105), B `--prebias` (their biases), C trunk
frozen (layers < 75), D an island (everything trains but block 80's weight and BatchNorm), E one weight deep in the trunk (conv 42, the
conv that computes layer 43: see tests/test_freeze_plan.py), H the last head conv alone (the other two heads need no gradient at all)."""
import copy
import os
import sys

import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model.loss import compute_loss
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.utils.synthetic import synthetic_targets

pytestmark = pytest.mark.gpu
HYP = {"giou": 0.1, "cls": 27.76, "cls_pw": 1.0, "obj": 20.35, "obj_pw": 1.0, "iou_t": 0.5, "ang_t": 3.1415926 / 12,
       "reg": 1.0, "fl_gamma": 0.5, "context_factor": 1.0}
SIZE, BS = 64, 2
HEADS = (81, 93, 105)
STATS = ("running_mean", "running_var", "num_batches_tracked")


def _well_conditioned(model, seed=5):
    """variance-preserving random conv weights, non-trivial BN affine (the helper of tests/test_train_engine_gpu.py)"""
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


def _trains(pattern, name):
    """does the parameter `name` (module_list.<layer>.<module>.<tensor>) train under `pattern`"""
    layer, rest = int(name.split(".")[1]), name.split(".", 2)[2]
    if pattern == "all":
        return True
    if pattern == "A":
        return layer in HEADS
    if pattern == "B":
        return layer in HEADS and rest == "Conv2d.bias"
    if pattern == "C":
        return layer >= 75
    if pattern == "D":
        return not (layer == 80 and rest in ("Conv2d.weight", "BatchNorm2d.weight", "BatchNorm2d.bias"))
    if pattern == "E":
        return layer == 42 and rest == "Conv2d.weight"
    if pattern == "H":
        return layer == 105
    raise KeyError(pattern)


def _freeze(model, pattern):
    for k, p in model.named_parameters():
        p.requires_grad = _trains(pattern, k)
    return model


def _step(model, x, tg):
    """one forward / loss / backward from cleared gradients -> (heads, loss, {name: grad} of the parameters that have one)"""
    model.zero_grad(set_to_none=True)
    pred = model(x)
    loss, items = compute_loss([p.float() for p in pred], tg.clone(), model, model.hyp)
    loss.backward()
    return ([p.detach().float().cpu() for p in pred], float(loss.detach()),
            {k: v.grad.detach().float().cpu().clone() for k, v in model.named_parameters() if v.grad is not None})


def _engine(model):
    engs = [e for e in model._engines.values() if hasattr(e, "bplan")]
    assert len(engs) == 1, "model._engines holds %d train engines" % len(engs)
    return engs[0]


def _same(got, want, names=None, what="", fused=False):
    """heads, loss and the gradients `names` (default: all of got's) bit for bit.  fused: the REPORTED loss of the graph-captured loss is
    summed with one fp32 atomic per workgroup, so its last bit depends on arrival order (the bound of
    tests/test_train_engine_gpu.py::test_no_graph_switch_runs_the_same_kernels_eagerly); nothing in the step reads it"""
    assert got[1] == want[1] or (fused and abs(got[1] - want[1]) <= 4e-7 * abs(want[1])), (what, got[1], want[1])
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b), (what, "head", float((a - b).abs().max()))
    names = set(got[2]) if names is None else names
    assert set(got[2]) == set(names), (what, sorted(set(got[2]) ^ set(names))[:6])
    for k in names:
        assert torch.equal(got[2][k], want[2][k]), (what, k, float((got[2][k] - want[2][k]).abs().max()), float(want[2][k].abs().max()))


class _Case(object):
    pass


@pytest.fixture(scope="module")
def case(cuda_dev):
    """the model, one batch, and the all-trainable step on a deep copy: computed once, never changed"""
    c = _Case()
    c.dev = cuda_dev
    base = _well_conditioned(Darknet(make_cfg.darknet53(SIZE, SIZE), dict(HYP))).to(cuda_dev).train()
    base.nc, base.arc = 1, "default"
    c.base = base
    c.x = torch.rand(BS, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).to(cuda_dev)
    c.tg = synthetic_targets(BS, seed=3, device=cuda_dev)
    ref = c.fresh()
    c.ref = _step(ref, c.x, c.tg)
    c.ref_stats = {k: v.detach().cpu().clone() for k, v in ref.state_dict().items() if k.endswith(STATS)}
    c.names = [k for k, _ in base.named_parameters()]
    assert len(c.ref_stats) == 3 * 72 and set(c.ref[2]) == set(c.names)
    del ref
    return c


def _fresh(self, pattern="all"):
    m = copy.deepcopy(self.base)
    m._engines = {}
    return _freeze(m, pattern)


_Case.fresh = _fresh


@pytest.mark.parametrize("pattern,count", [("A", 6), ("B", 3)])
def test_transfer_and_prebias_steps_give_the_bits_of_the_all_trainable_step(case, pattern, count):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train import make_optimizer
    m = case.fresh(pattern)
    want = [k for k in case.names if _trains(pattern, k)]
    assert len(want) == count
    got = _step(m, case.x, case.tg)
    _same(got, case.ref, want, pattern)
    named = dict(m.named_parameters())
    assert all(named[k].grad is None for k in case.names if k not in want)
    # the training forward is unchanged: frozen BatchNorm layers use batch statistics and update their running statistics
    sd = m.state_dict()
    for k, v in case.ref_stats.items():
        assert torch.equal(sd[k].cpu(), v), k
    # one FusedSGD step with weight decay: it skips what has no gradient
    before = {k: p.detach().clone() for k, p in named.items()}
    opt = make_optimizer(m, dict(HYP, lr0=0.01, momentum=0.9, weight_decay=0.05))
    assert type(opt).__name__ == "FusedSGD" and opt.param_groups[1]["weight_decay"] == 0.05
    opt.step()
    torch.cuda.synchronize()
    for k, p in named.items():
        assert torch.equal(p.detach(), before[k]) == (k not in want), k


@pytest.mark.parametrize("pattern", ["C", "D", "E", "H"])
def test_partial_backward_gives_the_bits_of_the_all_trainable_step(case, pattern):
    """the contributions a frozen pattern drops only ever went into gradients nobody reads: what remains keeps its order and its bits"""
    m = case.fresh(pattern)
    want = [k for k in case.names if _trains(pattern, k)]
    assert 0 < len(want) < len(case.names)
    got = _step(m, case.x, case.tg)
    _same(got, case.ref, want, pattern)
    assert all(p.grad is None for k, p in m.named_parameters() if k not in want)
    eng = _engine(m)
    ran = sorted(i for kind, i, _, _ in eng.bplan if kind == "conv")
    if pattern == "C":
        assert ran[0] == 75
    elif pattern == "H":
        assert ran == [105] and [kind for kind, _, _, _ in eng.bplan] == ["yolo", "conv"]
    elif pattern == "E":
        assert ran[0] == 42 and [b.i for b in eng.blocks if b.wgrad] == [42]
    else:
        assert ran[0] == 0 and [b.i for b in eng.blocks if not b.wgrad] == [80]


@pytest.mark.parametrize("pattern", ["A", "C"])
def test_frozen_steps_replay_from_graphs_with_the_same_bits(case, pattern):
    """four steps: two eager, the third captures the forward and backward graphs, the fourth replays them; and an engine built without
    graphs"""
    from rotate_yolov3_amd.model.train_engine import TrainEngine
    m = case.fresh(pattern)
    runs = [_step(m, case.x, case.tg) for _ in range(4)]
    eng = _engine(m)
    assert eng.g_fwd is not None and eng.g_bwd and all(g is not None for g in eng.g_bwd) and eng.graph_fallback is None
    for r, run in enumerate(runs):
        _same(run, runs[0], None, (pattern, r))
    _same(runs[0], case.ref, [k for k in case.names if _trains(pattern, k)], pattern)
    m2 = case.fresh(pattern)
    key, _ = m2._train_key(case.x.shape, case.dev)
    m2._engines[key] = TrainEngine(m2, case.x.shape, case.dev, use_graph=False)
    for r in range(3):
        _same(_step(m2, case.x, case.tg), runs[0], None, (pattern, "no graph", r))
    assert _engine(m2).g_fwd is None and _engine(m2).g_bwd == [None] and not _engine(m2).use_graph


def _count(eng, key):
    return sum(1 for b in eng.blocks if getattr(b, key) is not None and not (key == "dz" and b.bn is None))


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_a_frozen_engine_allocates_nothing_for_entries_that_do_not_run(case, pattern):
    """counts of tensors, nothing timed.  dz: the BatchNorm blocks' own buffer (a head conv's dz IS its dy, the head gradient).  Under
    --transfer the three head convs still compute weight gradients, so they -- and only they -- hold the split-K workspace of the
    batched reduce; under --prebias no block holds one."""
    full, m = case.fresh("all"), case.fresh(pattern)
    _step(full, case.x, case.tg)
    _step(m, case.x, case.tg)
    e_all, eng = _engine(full), _engine(m)
    assert e_all.batch_reduce and eng.batch_reduce
    assert (_count(e_all, "dz"), _count(e_all, "packed_d"), _count(e_all, "ws_w")) == (71, 74, 74)       # (layer 0: one pass, no dz, no dgrad)
    assert _count(eng, "dz") == 0 and _count(eng, "packed_d") == 0
    assert sorted(b.i for b in eng.blocks if b.ws_w is not None) == (list(HEADS) if pattern == "A" else [])
    assert eng._ws_w is None
    # no gradient view except the three heads'
    grads = set(v for v in eng._tplan.grd if v is not None)
    assert len(grads) == 3 and grads == set(eng._tplan.grd[i] for i in HEADS)
    assert len(set(v for v in e_all._tplan.grd if v is not None)) > 50
    for b in eng.blocks:
        assert b.xin_g is None and b.res_g is None and (b.dy is not None) == (b.i in HEADS)
        if b.i in HEADS:
            assert b.dz is b.dy
    assert len(eng._tplan.buffers) < len(e_all._tplan.buffers) - 50
    assert len(eng.static_grad) == (6 if pattern == "A" else 3) and len(e_all.static_grad) == len(case.names)
    assert len(eng.bplan) == 6 and len(e_all.bplan) == 75 + 2 + 3      # convs (their shortcuts folded in), upsamples, yolo layers


def _toggle_sequence(case, fused):
    """pattern A for two steps, everything trainable, back to A -> the three results that matter, and per step the head gradients the
    backward consumed (bf16 NHWC) with the loss items"""
    m = case.fresh("A")
    if fused:
        m.enable_fused_loss(capacity=32)
    out, heads = [], []

    def step():
        m.zero_grad(set_to_none=True)
        pred = m(case.x)
        loss, items = compute_loss([p.float() for p in pred], case.tg.clone(), m, m.hyp)
        loss.backward()
        eng = _engine(m)                                          # one train engine, whatever was toggled
        heads.append(([hg.detach().float().cpu() for _, hg in eng.head_pairs], items.detach().float().cpu()))
        assert (getattr(eng, "_fused_state", None) is not None) == fused
        return ([p.detach().float().cpu() for p in pred], float(loss.detach()),
                {k: v.grad.detach().float().cpu().clone() for k, v in m.named_parameters() if v.grad is not None})

    step()
    out.append(step())
    _freeze(m, "all")
    out.append(step())
    _freeze(m, "A")
    out.append(step())
    assert all(p.grad is None for k, p in m.named_parameters() if not _trains("A", k))
    return out, heads


def test_toggling_requires_grad_between_steps_works_in_both_directions(case):
    a_names = [k for k in case.names if _trains("A", k)]
    eager, heads_e = _toggle_sequence(case, fused=False)
    _same(eager[0], case.ref, a_names, "A")
    _same(eager[1], case.ref, case.names, "all after A")          # a fresh all-trainable model's step
    _same(eager[2], case.ref, a_names, "A again")
    # with the graph-captured loss: the same bits as a fresh all-trainable model with the fused loss ...
    ref = case.fresh("all")
    ref.enable_fused_loss(capacity=32)
    want = _step(ref, case.x, case.tg)
    assert getattr(_engine(ref), "_fused_state", None) is not None
    fused, heads_f = _toggle_sequence(case, fused=True)
    _same(fused[0], want, a_names, "fused A", fused=True)
    _same(fused[1], want, case.names, "fused all after A", fused=True)
    _same(fused[2], want, a_names, "fused A again", fused=True)
    # ... and against the eager loss mirror what tests/test_train_engine_gpu.py::test_fused_loss_graph_equals_eager_mirror allows: the loss
    # items to fp32 summation order, the head gradients at bf16 resolution
    for (hf, items_f), (he, items_e) in zip(heads_f, heads_e):
        assert torch.allclose(items_f, items_e, rtol=1e-4, atol=1e-6), (items_f, items_e)
        for a, b in zip(hf, he):
            assert torch.allclose(a, b, rtol=2 ** -7, atol=1e-9), float((a - b).abs().max())


def test_reducer_attached_after_freezing_takes_the_direct_sink(case):
    import torch.distributed as dist
    from rotate_yolov3_amd.dist import GradientAllReducer
    m = case.fresh("A")
    a_names = [k for k in case.names if _trains("A", k)]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    try:
        dp = GradientAllReducer(m, bucket_mb=32.0)
        assert len(dp.params) == 6
        pred = m(case.x)
        loss, _ = compute_loss([p.float() for p in pred], case.tg.clone(), m, m.hyp)
        loss.backward()
        dp.finish()
        eng = _engine(m)
        assert eng.direct and eng.static_flat is None and len(eng.static_grad) == 6
        named = dict(m.named_parameters())
        assert all(eng.static_grad[named[k]].data_ptr() == named[k].grad.data_ptr() for k in a_names)
        got = ([p.detach().float().cpu() for p in pred], float(loss.detach()),
               {k: v.grad.detach().float().cpu().clone() for k, v in named.items() if v.grad is not None})
        _same(got, case.ref, a_names, "reducer")
    finally:
        dist.destroy_process_group()
