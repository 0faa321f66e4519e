"""GPU tier: utils/fused_adam.FusedAdam (csrc/optim.hip: adam_batch_kernel, one launch for every tensor) against torch.optim.Adam.

The oracle is torch.optim.Adam on float64 CPU copies of the same fp32 inputs.  E_ref is the maximum absolute error against it, per tensor
and per quantity (p, exp_avg, exp_avg_sq), of torch.optim.Adam in fp32 on the same GPU; FusedAdam must stay within 2 * E_ref plus one fp32
ulp of that tensor's largest magnitude -- the last-bit differences between two correct fp32 evaluations, nothing larger has an explanation.
One scenario is run once per module (seven steps, three optimizers) and shared by the tests that read it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.utils.fused_adam import FusedAdam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 2 100 005 elements: more than the 1024 x 2048 at which the block count of a tensor stops growing, and a tail that is no multiple of 4
SHAPES = [(64, 32, 3, 3), (64,), (1,), (1000, 17), (5,), (3,), (2100005,)]
DECAYED, SCALED, NEVER, HUGE = 0, 1, 4, 5       # indices into SHAPES: weight_decay 5e-4; 1e-6 gradients on odd steps; no gradient; [0, 1e-30, 3e19]
QUANT = ("p", "exp_avg", "exp_avg_sq")


def _init():
    g = torch.Generator().manual_seed(11)
    return [torch.randn(s, generator=g) * 0.1 for s in SHAPES]


def _grad(step):
    """fp32 CPU gradients of step 1, 2, ...: None for the tensor that gets none (NEVER has its first gradient at step 7)"""
    g = torch.Generator().manual_seed(100 + step)
    out = []
    for k, s in enumerate(SHAPES):
        t = torch.randn(s, generator=g)
        if k == SCALED and step % 2 == 1:
            t = t * 1e-6
        if k == HUGE:
            t = torch.tensor([0.0, 1e-30, 3e19])
        out.append(None if k == NEVER and step < 7 else t)
    return out


def _make(cls, params, lr=1e-3, **kw):
    opt = cls([p for k, p in enumerate(params) if k != DECAYED], lr=lr, **kw)
    opt.add_param_group({"params": [params[DECAYED]], "weight_decay": 5e-4})
    return opt


def _snapshot(opt, params):
    snap = []
    for p in params:
        st = opt.state.get(p, {})
        # (clone: .double().cpu() of the fp64 CPU oracle is the tensor itself, which the next step rewrites)
        snap.append({"p": p.detach().double().cpu().clone(), "exp_avg": st["exp_avg"].double().cpu().clone() if "exp_avg" in st else None,
                     "exp_avg_sq": st["exp_avg_sq"].double().cpu().clone() if "exp_avg_sq" in st else None,
                     "step": float(st["step"]) if "step" in st else None, "version": p._version})
    return snap


def _scenario(classes, dev, dtype, nsteps=7, grad_mul=1.0, grad_scale=None, **kw):
    """classes[k]: the optimizer class of step k + 1; a change of class hands the state_dict() over.  lr is multiplied by 0.1 before step 4.
    -> {step: snapshot} for steps 3, 6 and 7, and the last optimizer with its parameters"""
    params = [torch.nn.Parameter(t.to(device=dev, dtype=dtype)) for t in _init()]
    opt, snaps = None, {}
    for step in range(1, nsteps + 1):
        cls = classes[step - 1]
        if opt is None or type(opt) is not cls:
            new = _make(cls, params, **kw)
            if opt is not None:
                new.load_state_dict(opt.state_dict())
            opt = new
            if grad_scale is not None:
                opt.grad_scale = grad_scale
        if step == 4:
            for group in opt.param_groups:
                group["lr"] *= 0.1
        for p, g in zip(params, _grad(step)):
            p.grad = None if g is None else (g * grad_mul).to(device=dev, dtype=dtype)
        opt.step()
        if step in (3, 6, 7):
            snaps[step] = _snapshot(opt, params)
    return snaps, opt, params


@pytest.fixture(scope="module")
def runs(cuda_dev):
    T, F = torch.optim.Adam, FusedAdam
    out = {"oracle": _scenario([T] * 7, torch.device("cpu"), torch.float64)[0], "torch": _scenario([T] * 7, cuda_dev, torch.float32)[0]}
    out["fused"], out["fused_opt"], out["fused_params"] = _scenario([F] * 7, cuda_dev, torch.float32)
    torch.cuda.synchronize()
    return out


def _meets_the_bar(got, ref32, oracle, label):
    bad = []
    for k, s in enumerate(SHAPES):
        for q in QUANT:
            o, r, g = oracle[k][q], ref32[k][q], got[k][q]
            assert (o is None) == (r is None) == (g is None), (label, s, q)
            if o is None:
                continue
            e, e_ref = (g - o).abs().max().item(), (r - o).abs().max().item()
            ulp = float(np.spacing(np.float32(o.abs().max().item())))
            print("%s %-14s %-10s  fused %.3e  torch fp32 (E_ref) %.3e  ulp %.3e" % (label, s, q, e, e_ref, ulp))
            if not e <= 2 * e_ref + ulp:
                bad.append((s, q, e, e_ref, ulp))
    assert not bad, bad


def test_parity_with_torch_adam_in_fp64_over_six_steps(runs):
    """every path of the kernel in one launch: 16-byte body and 4-byte tail, a tensor at its block cap, 1- and 3-element tensors, a group
    with weight decay, an lr change, 1e-6 gradients and a 3e19 gradient whose square overflows fp32 (((1 - beta2) * d) * d does not)"""
    _meets_the_bar(runs["fused"][6], runs["torch"][6], runs["oracle"][6], "step 6")
    assert [s["step"] for s in runs["fused"][6]] == [s["step"] for s in runs["torch"][6]] == [6.0] * 4 + [None] + [6.0] * 2
    # The 3e19 gradient.  On the GPU torch's own fp32 step evaluates value * (d * d) in _foreach_addcmul_ (its CPU kernel and the fp64
    # oracle do not overflow), so its exp_avg_sq there is inf, E_ref is inf and the bar above says nothing about that element.  The
    # kernel's ((1 - beta2) * d) * d stays finite; it gets a bar of its own: four roundings per step (v * beta2, (1 - beta2) * d, * d,
    # the sum), each at most half an ulp of a value no larger than the final one, six steps -> 12 ulp.
    huge, want = runs["fused"][6][HUGE], runs["oracle"][6][HUGE]
    assert all(torch.isfinite(huge[q]).all() for q in QUANT)
    e, ulp = (huge["exp_avg_sq"] - want["exp_avg_sq"]).abs().max().item(), float(np.spacing(np.float32(want["exp_avg_sq"].max().item())))
    print("exp_avg_sq of the 3e19 gradient: fused %.6e  fp64 %.6e  error %.2f ulp; torch fp32 on this GPU: %s"
          % (huge["exp_avg_sq"][2].item(), want["exp_avg_sq"][2].item(), e / ulp, runs["torch"][6][HUGE]["exp_avg_sq"][2].item()))
    assert 1e36 < huge["exp_avg_sq"][2].item() < 1e37 and huge["exp_avg_sq"][0].item() == 0.0 and e <= 12 * ulp


def test_a_parameter_without_gradient_is_left_alone_and_starts_its_own_step_count_later(runs):
    six, seven = runs["fused"][6], runs["fused"][7]
    assert torch.equal(six[NEVER]["p"], _init()[NEVER].double()), "a parameter with no gradient changed"
    assert six[NEVER]["exp_avg"] is None and six[NEVER]["step"] is None and six[NEVER]["version"] == 0
    # step 7: its first gradient -- two (group, step count) rows in one launch
    assert [s["step"] for s in seven] == [7.0] * 4 + [1.0] + [7.0] * 2 == [s["step"] for s in runs["torch"][7]]
    assert not torch.equal(seven[NEVER]["p"], six[NEVER]["p"])
    _meets_the_bar(seven, runs["torch"][7], runs["oracle"][7], "step 7")


@pytest.mark.parametrize("offsets", [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 2, 3)])
def test_unaligned_views_give_the_same_bits_and_nothing_outside_them_is_written(cuda_dev, offsets):
    """p, g, exp_avg and exp_avg_sq as views into flat buffers (what the gradients of dist.py's buckets are) at element offsets 0..3 from
    a 16-byte boundary, sentinels on both sides, against the step on separately allocated tensors"""
    GUARD, SENTINEL = 8, 777.0
    gen = torch.Generator().manual_seed(5)
    flat, views, plain = [], [], []
    for n in (2049, 5):
        vals = [torch.randn(n, generator=gen) for _ in range(2)] + [torch.zeros(n), torch.zeros(n)]
        bufs = [torch.full((GUARD + off + n + GUARD,), SENTINEL, device=cuda_dev) for off in offsets]
        assert all(b.data_ptr() % 16 == 0 for b in bufs)
        vs = [b[GUARD + off:GUARD + off + n] for b, off in zip(bufs, offsets)]
        for v, x in zip(vs, vals):
            v.copy_(x)
        assert [v.data_ptr() % 16 for v in vs] == [4 * off for off in offsets]
        flat.append((bufs, n))
        views.append(vs)
        plain.append([x.clone().to(cuda_dev) for x in vals])

    def run(sets):
        ps = [torch.nn.Parameter(s[0]) for s in sets]
        opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-3)
        for p, s in zip(ps, sets):
            assert p.data_ptr() == s[0].data_ptr()
            p.grad = s[1]
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": s[2], "exp_avg_sq": s[3]}
        for _ in range(2):
            opt.step()
        return ps
    run(views)
    run(plain)
    torch.cuda.synchronize()
    for vs, ps, (bufs, n) in zip(views, plain, flat):
        for q in (0, 2, 3):
            assert torch.equal(vs[q], ps[q]), (n, q)
        assert not torch.equal(ps[2], torch.zeros_like(ps[2]))
        for b, off in zip(bufs, offsets):
            assert (b[:GUARD + off] == SENTINEL).all() and (b[GUARD + off + n:] == SENTINEL).all(), (n, off)


def test_grad_scale_folds_the_data_parallel_average_into_the_step(cuda_dev, runs):
    snaps, opt, _ = _scenario([FusedAdam] * 6, cuda_dev, torch.float32, nsteps=6, grad_mul=2.0, grad_scale=0.5)
    assert opt.grad_scale == 0.5
    for k, (a, b) in enumerate(zip(snaps[6], runs["fused"][6])):
        for q in QUANT:
            assert (a[q] is None and b[q] is None) or torch.equal(a[q], b[q]), (SHAPES[k], q)


def test_two_runs_are_bit_equal_and_every_stepped_parameter_has_a_new_version(cuda_dev, runs):
    snaps, _, params = _scenario([FusedAdam] * 3, cuda_dev, torch.float32, nsteps=3)
    for k, (a, b) in enumerate(zip(snaps[3], runs["fused"][3])):
        for q in QUANT:
            assert (a[q] is None and b[q] is None) or torch.equal(a[q], b[q]), (SHAPES[k], q)
    # a fresh Parameter is at version 0; each step bumps the ones it wrote
    assert [p._version for p in params] == [3, 3, 3, 3, 0, 3, 3]
    assert [s["version"] for s in runs["fused"][7]] == [7, 7, 7, 7, 1, 7, 7]


@pytest.mark.parametrize("first,second", [(torch.optim.Adam, FusedAdam), (FusedAdam, torch.optim.Adam)])
def test_state_dict_moves_between_torch_adam_and_fused_adam(cuda_dev, runs, first, second):
    snaps, opt, params = _scenario([first] * 3 + [second] * 3, cuda_dev, torch.float32, nsteps=6)
    assert type(opt) is second
    _meets_the_bar(snaps[6], runs["torch"][6], runs["oracle"][6], "%s -> %s" % (first.__name__, second.__name__))
    ref = _scenario([torch.optim.Adam] * 1, cuda_dev, torch.float32, nsteps=1)[1]
    want = next(iter(ref.state.values()))
    for k, p in enumerate(params):
        st = opt.state.get(p, {})
        if k == NEVER:
            assert len(st) == 0
            continue
        assert list(st) == list(want) == ["step", "exp_avg", "exp_avg_sq"]
        assert st["step"].dtype == want["step"].dtype == torch.float32 and st["step"].device == want["step"].device == torch.device("cpu")
        assert float(st["step"]) == 6.0 and st["exp_avg"].device == p.device
    a, b = opt.state_dict(), _make(first, params).state_dict()
    assert [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]


def test_the_large_weight_lerp_form(cuda_dev):
    """beta1 < 0.5: ATen's lerp switches to end - (end - self) * (1 - weight); so does the kernel"""
    shape, g = (1000, 17), torch.Generator().manual_seed(3)
    p0, grads = torch.randn(shape, generator=g) * 0.1, [torch.randn(shape, generator=g) for _ in range(3)]
    res = []
    for cls, dev, dt in ((torch.optim.Adam, torch.device("cpu"), torch.float64), (torch.optim.Adam, cuda_dev, torch.float32),
                         (FusedAdam, cuda_dev, torch.float32)):
        p = torch.nn.Parameter(p0.to(device=dev, dtype=dt))
        opt = cls([p], lr=1e-3, betas=(0.3, 0.9), weight_decay=1e-2)
        for gr in grads:
            p.grad = gr.to(device=dev, dtype=dt)
            opt.step()
        res.append([p.detach().double().cpu(), opt.state[p]["exp_avg"].double().cpu(), opt.state[p]["exp_avg_sq"].double().cpu()])
    for q in range(3):
        e, e_ref = (res[2][q] - res[0][q]).abs().max().item(), (res[1][q] - res[0][q]).abs().max().item()
        ulp = float(np.spacing(np.float32(res[0][q].abs().max().item())))
        print("%-10s fused %.3e  torch fp32 %.3e  ulp %.3e" % (QUANT[q], e, e_ref, ulp))
        assert e <= 2 * e_ref + ulp


def test_eval_after_adam_training_steps_sees_the_updated_weights(cuda_dev):
    """tests/test_train_engine_gpu.py: test_eval_after_training_step_sees_the_updated_weights, with FusedAdam: the cached eval engine must
    notice that the kernel rewrote the parameters behind autograd's back (the version bump)"""
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.model.loss import compute_loss
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.utils.synthetic import synthetic_targets
    from tests.test_train_engine_gpu import HYP, _well_conditioned
    torch.manual_seed(1)
    m = _well_conditioned(Darknet(make_cfg.darknet53(64, 64), dict(HYP))).to(cuda_dev)
    m.nc, m.arc = 1, "default"
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(cuda_dev)
    tg = synthetic_targets(4, seed=4, device=cuda_dev)
    m.eval()
    with torch.no_grad():
        io0 = m(x)[1][0].clone()
    opt = FusedAdam(m.parameters(), lr=1e-3)
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


def test_make_optimizer_picks_fused_adam_on_a_gpu(cuda_dev):
    sys.path.insert(0, ROOT)
    from train import make_optimizer
    from rotate_yolov3_amd.model.models import Darknet
    from tests.test_train_engine_gpu import HYP, MINI_CFG
    hyp = dict(HYP, lr0=1e-3, momentum=0.9, weight_decay=5e-4)
    m = Darknet(MINI_CFG, hyp).to(cuda_dev)
    opt = make_optimizer(m, hyp, adam=True)
    assert type(opt) is FusedAdam and len(opt.param_groups) == 2
    assert opt.param_groups[0]["weight_decay"] == 0 and opt.param_groups[1]["weight_decay"] == 5e-4 and opt.param_groups[0]["lr"] == 1e-3
    assert type(make_optimizer(m, hyp, adam=True, fused=False)) is torch.optim.Adam
    m.half()
    assert type(make_optimizer(m, hyp, adam=True)) is torch.optim.Adam


HYP_FILE = ("giou: 0.1\ncls: 27.76\ncls_pw: 1.0\nobj: 20.35\nobj_pw: 1.0\niou_t: 0.5\nang_t: 3.1415926/12\nreg: 1.0\nfl_gamma: 0.5\n"
            "context_factor: 1.0\nlr0: 0.0001\nmultiplier:10\nwarm_epoch:1\nmomentum: 0.97\nweight_decay: 0.0004569\nepochs: 1\n"
            "batch_size: 2\nsave_interval: 1\ntest_interval: 5\n")


def test_train_py_adam_saves_and_reloads_the_optimizer_state(cuda_dev, tmp_path):
    from tests.test_train_engine_gpu import MINI_CFG
    (tmp_path / "mini.cfg").write_text(MINI_CFG)
    (tmp_path / "hyp.py").write_text(HYP_FILE)
    wdir = tmp_path / "w"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--adam", "--device", "0", "--img-size", "64", "--synthetic", "4", "--epochs", "3",
           "--cfg", str(tmp_path / "mini.cfg"), "--hyp", str(tmp_path / "hyp.py"), "--wdir", str(wdir)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "non-finite" not in r.stdout
    ck = torch.load(str(wdir / "backup1.pt"), map_location="cpu")
    state = ck["optimizer"]["state"]
    assert len(state) > 0 and all(list(st) == ["step", "exp_avg", "exp_avg_sq"] for st in state.values())
    assert all(float(st["step"]) == 4.0 for st in state.values())          # two epochs of two steps
    assert len(ck["optimizer"]["param_groups"]) == 2 and "betas" in ck["optimizer"]["param_groups"][0]
    r = subprocess.run(cmd + ["--weights", str(wdir / "backup1.pt")], cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "non-finite" not in r.stdout and "3 epochs completed" in r.stdout
    ck2 = torch.load(str(wdir / "backup1.pt"), map_location="cpu")
    assert all(float(st["step"]) == 8.0 for st in ck2["optimizer"]["state"].values())      # the loaded counts went on
