"""The detection heads of the training step.

Forward: ryolo_conv_head_decode_store -- the head's 1x1 conv, the raw p rows and the store of the bf16 head tensor as one launch
(csrc/conv_pw.hip MODE 5) -- against the two launches it replaces, ryolo_conv2d_bn_act + ryolo_yolo_decode (p only): bit for bit.
Engine: a TrainEngine with both head changes (that launch, and the head bias gradients taken from the loss's dense pass,
tests/test_head_bias_fold_gpu.py) against one with RYOLO_HEAD_DECODE=0 RYOLO_HEAD_BIAS_FOLD=0 on a copy of the model."""
import copy
import ctypes as C

import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model import hip_train_ops as tr
from rotate_yolov3_amd.model.loss import compute_loss
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.utils.synthetic import synthetic_targets

pytestmark = pytest.mark.gpu
HYP = {"giou": 0.1, "cls": 27.76, "cls_pw": 1.0, "obj": 20.35, "obj_pw": 1.0, "iou_t": 0.5, "ang_t": 3.1415926 / 12,
       "reg": 1.0, "fl_gamma": 0.5, "context_factor": 1.0, "riou": 1}
SENTINEL = 3.0


def _desc(N, H, W, cin, cout, in_cs, out_cs):
    return ops.ConvDesc(N, H, W, cin, cout, 1, 1, 0, in_cs, out_cs, 0, 0, 0.0, 1, 0)


# C_in 256 / 1024: two channel blocks of 256 (block 1 starts at channel 252: 4-B edge stores on both sides of the seam) and four of 128
# (seams at 126, 252, 378); 2 x 5 x 5 = 50 pixels: fewer rows than one workgroup's 64-row block; 2 x 13 x 11 = 286: four full row blocks
# and a tail of 30; head pixel stride equal to C and larger than C; na 72 x no 7 = 504 (the flagship heads) and 24 x 8 = 192 (one block
# of 256, or two of 128 with an aligned seam)
@pytest.mark.parametrize("cin", [256, 1024])
@pytest.mark.parametrize("grid", [(2, 5, 5), (2, 13, 11)])
@pytest.mark.parametrize("na,no,head_cs", [(72, 7, 504), (72, 7, 512), (24, 8, 192)])
def test_fused_head_equals_conv_then_decode(cuda_dev, cin, grid, na, no, head_cs):
    dev = cuda_dev
    L = _lib.lib()
    N, H, W = grid
    cout = na * no
    g = torch.Generator().manual_seed(cin + H + na)
    in_cs = cin + 64                                                   # the input is a channel slice of a wider buffer
    x = torch.randn(N, H, W, in_cs, generator=g).to(dev).to(torch.bfloat16)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5).to(dev)
    cp = max(ops.cpad(cout), 512)
    packed = ops.pack_weights(wt, cin_pad=cin)
    ones = ops.pad_vec(torch.ones(cout, device=dev), cp)
    bias = ops.pad_vec((torch.randn(cout, generator=g) * 0.3).to(dev), cp)
    d = _desc(N, H, W, cin, cout, in_cs, cout)
    assert L.ryolo_conv_head_decode_supported(C.byref(d), na, no) == 1
    anchors = torch.ones(na, 3, device=dev)

    # the separate path: conv into the head buffer (channels >= C_out of a wider pixel stride stay as they were), p-only decode
    head0 = torch.full((N, H, W, head_cs), SENTINEL, dtype=torch.bfloat16, device=dev)
    p0 = torch.full((N, na, H, W, no), -5.0, device=dev)
    d0 = _desc(N, H, W, cin, cout, in_cs, head_cs)
    _lib.check(L.ryolo_conv2d_bn_act(C.byref(d0), x.data_ptr(), packed.data_ptr(), ones.data_ptr(), bias.data_ptr(), None, head0.data_ptr(),
                                     _lib.stream_ptr(dev)), "ryolo_conv2d_bn_act")
    _lib.check(L.ryolo_yolo_decode(head0.data_ptr(), head_cs, N, H, W, na, no, anchors.data_ptr(), 32.0, 1.0, 0, None, na * H * W, 0,
                                   p0.data_ptr(), _lib.stream_ptr(dev)), "ryolo_yolo_decode")
    # one launch
    head1 = torch.full((N, H, W, head_cs), SENTINEL, dtype=torch.bfloat16, device=dev)
    p1 = torch.full((N, na, H, W, no), -5.0, device=dev)
    tr.conv_head_decode_store(dict(desc=(N, H, W, cin, cout, 1, 1, 0, in_cs, cout, 0, 0, 0.0, 1, 0), na=na, no=no),
                              x[..., :cin], packed, ones, bias, head1[..., :cout], p1)
    torch.cuda.synchronize()
    assert bool((p0 != -5.0).all()) and float(head0[..., :cout].float().abs().max()) > 0.5
    assert torch.equal(p1, p0), float((p1 - p0).abs().max())
    assert torch.equal(head1.view(torch.int16), head0.view(torch.int16)), float((head1.float() - head0.float()).abs().max())
    if head_cs > cout:                                                 # padding channels: as the separate path leaves them
        assert bool((head1[..., cout:] == SENTINEL).all()) and bool((head0[..., cout:] == SENTINEL).all())


def test_a_576_channel_head_is_not_served(cuda_dev):
    """nc = 2: 72 x 8 = 576 channels, more than the 512 one workgroup's tile holds: the query says no, the entry point refuses"""
    L = _lib.lib()
    d = _desc(2, 5, 5, 256, 576, 256, 576)
    assert L.ryolo_conv_head_decode_supported(C.byref(d), 72, 8) == 0
    fake = torch.zeros(16, device=cuda_dev)
    assert L.ryolo_conv_head_decode_store(C.byref(d), fake.data_ptr(), fake.data_ptr(), fake.data_ptr(), fake.data_ptr(), 72, 8,
                                          fake.data_ptr(), 576, fake.data_ptr(), None) != 0


def _well_conditioned(model, seed=5):
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed)
        for name, t in model.state_dict().items():
            if t.dim() == 4:
                t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * (6.0 / t[0].numel()) ** 0.5)
            elif name.endswith("BatchNorm2d.weight"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("BatchNorm2d.bias") or (t.dim() == 1 and name.endswith("Conv2d.bias")):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
    return model


def _step(model, x, targets):
    model.zero_grad(set_to_none=True)
    pred = model(x)
    loss, items = compute_loss([p.float() for p in pred], targets.clone(), model, model.hyp)
    loss.backward()
    return ([p.detach().float().cpu() for p in pred], float(loss.detach()),
            {k: v.grad.detach().float().cpu().clone() for k, v in model.named_parameters() if v.grad is not None})


def _engine(m):
    return [e for e in m._engines.values() if hasattr(e, "_segs")][0]


def test_engine_with_fused_heads_equals_the_separate_passes(cuda_dev, monkeypatch):
    """darknet53 at 96^2, bs 2, fused loss, four steps (eager, eager, capture, replay): pred, every parameter gradient and every state
    entry bit for bit, except the three head biases' gradients, which differ by fp32 summation order only -- bar: 1e-3 of the
    per-channel sum of magnitudes of the head gradient (tests/test_train_engine_blocks_gpu.py).  Steps 3 and 4 of a second run of the
    new path give the bits of the first.
    The REPORTED loss is compared to 4e-7 relative, not bit for bit: the dense loss kernels add their per-workgroup sums into it with one
    fp32 atomic each, so its last bit depends on arrival order in any two runs (tests/test_train_engine_gpu.py::
    test_no_graph_switch_runs_the_same_kernels_eagerly documents the same); nothing the step computes reads it."""
    dev = cuda_dev
    size, bs = 96, 2
    cfg = make_cfg.darknet53(size, size)
    m_new = _well_conditioned(Darknet(cfg, dict(HYP))).to(dev).train()
    m_new.nc, m_new.arc = 1, "default"
    m_old, m_new2 = copy.deepcopy(m_new), copy.deepcopy(m_new)
    for m in (m_new, m_old, m_new2):
        m._engines = {}
        m.enable_fused_loss(capacity=64)
    x = torch.rand(bs, 3, size, size, generator=torch.Generator().manual_seed(3)).to(dev)
    tg = synthetic_targets(bs, seed=6, device=dev)

    with _lib.trace_calls() as log:
        new = [_step(m_new, x, tg)]
    names = [c[0] for c in log]
    assert names.count("ryolo_conv_head_decode_store") == 3 and "ryolo_yolo_decode" not in names
    new += [_step(m_new, x, tg) for _ in range(3)]
    e_new = _engine(m_new)
    heads = [b for b in e_new.blocks if b.head_k is not None]
    assert len(heads) == 3 and all(b.head_fused for b in heads)
    assert e_new._g_bwd_fold == (True, True, True) and all(gr is not None for gr in e_new.g_bwd) and e_new.g_fwd is not None
    by_id = {id(q): k for k, q in m_new.named_parameters()}
    bias_names = {by_id[id(b.conv.bias)]: b.head_k for b in heads}

    monkeypatch.setenv("RYOLO_HEAD_DECODE", "0")
    monkeypatch.setenv("RYOLO_HEAD_BIAS_FOLD", "0")
    with _lib.trace_calls() as log:
        old = [_step(m_old, x, tg)]
    names = [c[0] for c in log]
    assert names.count("ryolo_yolo_decode") == 3 and "ryolo_conv_head_decode_store" not in names and "ryolo_head_bias_finalize" not in names
    old += [_step(m_old, x, tg) for _ in range(3)]
    e_old = _engine(m_old)
    assert not e_old.head_bias_fold and not any(b.head_fused for b in e_old.blocks) and e_old._g_bwd_fold == (False, False, False)
    monkeypatch.delenv("RYOLO_HEAD_DECODE")
    monkeypatch.delenv("RYOLO_HEAD_BIAS_FOLD")
    new2 = [_step(m_new2, x, tg) for _ in range(4)]
    torch.cuda.synchronize()

    bars = {k: 1e-3 * e_old.head_pairs[k][1].float().abs().sum((0, 1, 2)).cpu() + 1e-6 for k in range(3)}
    for s, (a, b) in enumerate(zip(new, old)):
        assert abs(a[1] - b[1]) <= 4e-7 * abs(b[1]), (s, a[1], b[1])
        for pa, pb in zip(a[0], b[0]):
            assert torch.equal(pa, pb), s
        assert a[2].keys() == b[2].keys()
        for k in b[2]:
            if k in bias_names:
                err = (a[2][k] - b[2][k]).abs()
                print("step %d %s: max |dbias| %.3e, max err %.3e, max err / bar %.3e" % (
                    s, k, float(b[2][k].abs().max()), float(err.max()), float((err / bars[bias_names[k]]).max())))
                assert bool((err <= bars[bias_names[k]]).all()), (s, k)
            else:
                assert torch.equal(a[2][k], b[2][k]), (s, k)
    sd_new, sd_old = m_new.state_dict(), m_old.state_dict()
    for k in sd_old:
        assert torch.equal(sd_new[k], sd_old[k]), k
    for s in (2, 3):                                                   # capture, replay: the bits of a second run
        assert abs(new[s][1] - new2[s][1]) <= 4e-7 * abs(new[s][1])
        for pa, pb in zip(new[s][0], new2[s][0]):
            assert torch.equal(pa, pb)
        for k in new[s][2]:
            assert torch.equal(new[s][2][k], new2[s][2][k]), (s, k)


def test_engine_takes_two_launches_for_a_576_channel_head(cuda_dev):
    """classes = 2: no = 8, 72 x 8 = 576-channel heads: the training engine keeps conv + decode (and still folds nothing it cannot:
    the 576-channel bias rows are not served either), and the step runs"""
    dev = cuda_dev
    hyp = dict(HYP)
    m = _well_conditioned(Darknet(make_cfg.darknet53(96, 96, classes=2), hyp)).to(dev).train()
    m.nc, m.arc = 2, "default"
    m._engines = {}
    m.enable_fused_loss(capacity=64)
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(3)).to(dev)
    tg = synthetic_targets(2, seed=6, device=dev)
    with _lib.trace_calls() as log:
        _step(m, x, tg)
    names = [c[0] for c in log]
    assert names.count("ryolo_yolo_decode") == 3 and "ryolo_conv_head_decode_store" not in names
    assert "ryolo_head_bias_finalize" not in names and names.count("ryolo_bn_act_bwd") >= 3
    eng = _engine(m)
    assert not any(b.head_fused for b in eng.blocks)
