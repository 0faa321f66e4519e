"""The detection heads' bias gradient out of the loss's dense pass (csrc/loss.hip: ryolo_yolo_loss_nhwc_bias writes rows of
per-channel sums of the head gradient it stores; csrc/train.hip: ryolo_head_bias_finalize turns the rows into dbias += g * sum)
against the pass it replaces: ryolo_bn_act_bwd in its bias form over the head gradient the loss wrote.

Bar: the per-operator bar of tests/test_train_engine_blocks_gpu.py for dbias, 1e-3 of the per-channel sum of magnitudes (+ 1e-6).
For an upstream gradient of 1 the test asks more: the same bits -- rows and finalize add the same bf16 values in the separate pass's
order (a training run then computes what it computed with the separate pass, step after step).

Shapes: 72 anchors x 7 = 504 channels (the flagship heads, 512-wide rows), and the two smallest heads the NHWC loss serves, 3 x 8 = 24
and 8 x 7 = 56 channels (128-wide rows).  A 3 x 7 = 21-channel head is not a multiple of 8 channels: neither the NHWC loss nor
ryolo_bn_act_bwd accepts it (the engine converts such a head's fp32 gradient and runs no NHWC loss), which
test_a_21_channel_head_is_refused_by_both_paths pins.  Grids: 2 x 13 x 11 (286 pixels: three slabs of 128 pixels, the last one short; 8 pixel lanes per
slab at 504 channels, 128 at 24: lanes without a pixel) and 1 x 1 x 1 (one pixel)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HYP = {"giou": 0.7, "cls": 1.3, "cls_pw": 1.5, "obj": 2.1, "obj_pw": 0.8, "iou_t": 0.3, "ang_t": math.pi / 4, "reg": 1.1,
       "context_factor": 1.0}


def _head(dev, na, no, bs, ny, nx, positives, seed):
    """(head bf16 NHWC, p fp32, target dict): two positives share one cell (same anchor), one sits in the last cell with the last
    anchor, one more anchor at the first cell; positives=False: a head that received no target."""
    g = torch.Generator().manual_seed(seed)
    C = na * no
    head = (torch.randn(bs, ny, nx, C, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    p = head.float().reshape(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4).contiguous()
    NT = 8
    w = torch.zeros(na, NT)
    b, gj, gi = torch.zeros(NT, dtype=torch.long), torch.zeros(NT, dtype=torch.long), torch.zeros(NT, dtype=torch.long)
    cy, cx = min(3, ny - 1), min(4, nx - 1)
    gj[0], gi[0] = cy, cx
    gj[1], gi[1] = cy, cx
    b[2], gj[2], gi[2] = bs - 1, ny - 1, nx - 1
    if positives:
        w[0, 0] = w[0, 1] = 1.0
        w[1, 0] = 1.0
        w[na - 1, 2] = 1.0
    av = torch.cat((0.5 + 2.0 * torch.rand(na, 2, generator=g), (torch.rand(na, 1, generator=g) - 0.5)), 1)
    hd = dict(w=w, b=b, gj=gj, gi=gi, cls=torch.randint(0, max(no - 6, 1), (NT,), generator=g),
              gxy=torch.rand(NT, 2, generator=g), gwh=0.5 + 2.0 * torch.rand(NT, 2, generator=g),
              ga=(torch.rand(NT, generator=g) - 0.5), av=av)
    hd = {k: v.to(dev) for k, v in hd.items()}
    hd['npos'] = hd['w'].sum().reshape(1)
    return head, p, hd


CASES = [(72, 7, 2, 13, 11, True), (72, 7, 2, 13, 11, False), (72, 7, 1, 1, 1, True),
         (3, 8, 2, 13, 11, True), (3, 8, 1, 1, 1, True), (8, 7, 2, 13, 11, True)]


@pytest.mark.parametrize("na,no,bs,ny,nx,positives", CASES)
def test_folded_head_bias_gradient_equals_the_separate_pass(cuda_dev, na, no, bs, ny, nx, positives):
    from rotate_yolov3_amd.model import hip_train_ops as tr
    from rotate_yolov3_amd.model.hip_ops import cpad
    dev = cuda_dev
    nc = max(no - 6, 1)
    C = na * no
    head, p, hd = _head(dev, na, no, bs, ny, nx, positives, seed=na * 100 + ny)
    npix = bs * ny * nx
    rows = tr.yolo_loss_bias_rows(p)
    assert rows > 0

    def loss(part):
        scratch = torch.zeros_like(p)
        hg = torch.full((bs, ny, nx, C), 3.0, dtype=torch.bfloat16, device=dev)
        it = torch.zeros(4, device=dev)
        tr.yolo_loss_head_nhwc(head, p, hd, nc, HYP, tr.yolo_loss_bitmap(p), scratch, hg, it, bias_part=part)
        assert float(scratch.abs().max()) == 0.0
        return hg, it

    hg0, it0 = loss(None)
    part = torch.full((rows, cpad(C)), float('nan'), device=dev)        # every row is written: no clearing needed
    hg1, it1 = loss(part)
    torch.cuda.synchronize()
    # the head gradient is byte-identical with and without the fold; the loss items add the same terms in another partition
    assert torch.equal(hg0.view(torch.int16), hg1.view(torch.int16))
    assert torch.allclose(it0, it1, rtol=2e-5, atol=1e-6)
    assert bool(torch.isfinite(part).all()) and float(part[:, C:].abs().max() if cpad(C) > C else 0.0) == 0.0
    if positives:        # the positives reached the gradient (columns other than the objectness one are non-zero somewhere)
        cols = hg0.float().reshape(-1, na, no).abs().sum((0, 1))
        assert int((cols > 0).sum()) > 1
    ws_old = torch.empty(max(tr.bn_bwd_ws_bytes(npix, C), 256), dtype=torch.uint8, device=dev)
    ws_new = torch.empty(max(tr.head_bias_ws_bytes(npix, C), 256), dtype=torch.uint8, device=dev)
    fill = torch.linspace(-1.0, 1.0, C, device=dev)
    for scale in (1.0, 0.5):
        gs = torch.full((1,), scale, device=dev)
        dy = hg0.clone()
        tr.scale_bf16_if(gs, dy)                      # what the fused loss's backward does to the head gradient
        want = fill.clone()
        tr.bn_act_bwd(head, dy, None, 0, None, None, None, want, None, ws_old)
        got = [fill.clone(), fill.clone()]
        for acc in got:                               # += into a pre-filled accumulator, twice: bit-reproducible
            tr.head_bias_finalize(part, npix, C, gs, acc, ws_new)
        torch.cuda.synchronize()
        assert torch.equal(got[0], got[1])
        mag = dy.float().abs().sum((0, 1, 2))
        bar = 1e-3 * mag + 1e-6
        err = (got[0] - want).abs()
        print("C=%d npix=%d scale=%g: max |dbias err| %.3e, max err / bar %.3e, max |dbias| %.3e" % (
            C, npix, scale, float(err.max()), float((err / bar).max()), float((want - fill).abs().max())))
        assert bool((err <= bar).all()), float((err / bar).max())
        # ... and it is an accumulation of the scaled sum: exact in the scale for a power of two
        if scale == 1.0:
            assert torch.equal(got[0], want), float(err.max())         # the separate pass's order: its bits
            unit = got[0] - fill
        else:
            assert torch.allclose(got[0] - fill, unit * scale, rtol=1e-5, atol=1e-6)
    # a second loss call into the same rows gives the same rows (no atomics, fixed order)
    part2 = torch.zeros_like(part)
    loss(part2)
    torch.cuda.synchronize()
    assert torch.equal(part, part2)


def test_a_21_channel_head_is_refused_by_both_paths(cuda_dev):
    """3 anchors x 7 = 21 channels is no multiple of the 8-channel chunks: no rows, and the NHWC loss (with or without rows) and the
    separate bias pass both return an error instead of computing -- the fold can not be reached for such a head."""
    from rotate_yolov3_amd.model import hip_train_ops as tr
    dev = cuda_dev
    head, p, hd = _head(dev, 3, 8, 1, 2, 2, True, seed=1)
    p21 = p[..., :7].contiguous()
    assert tr.yolo_loss_bias_rows(p21) == 0
    head21 = torch.zeros(1, 2, 2, 21, dtype=torch.bfloat16, device=dev)
    hg = torch.zeros_like(head21)
    for part in (None, torch.zeros(128, 128, device=dev)):
        with pytest.raises((RuntimeError, ValueError)):
            tr.yolo_loss_head_nhwc(head21, p21, hd, 1, HYP, tr.yolo_loss_bitmap(p21), torch.zeros_like(p21), hg, torch.zeros(4, device=dev),
                                   bias_part=part)
    with pytest.raises(RuntimeError):
        tr.bn_act_bwd(head21, hg, None, 0, None, None, None, torch.zeros(21, device=dev), None, torch.empty(4096, dtype=torch.uint8, device=dev))
    # rows are refused for the other arcs and for more than 512 channels too
    assert tr.yolo_loss_bias_rows(torch.empty(1, 72, 2, 2, 8, device=dev)) == 0
    assert tr.yolo_loss_bias_rows(p, arc=tr.ARC_FOCAL) == 0
