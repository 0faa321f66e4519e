"""GPU tier: one parity case per edge class of the dispatch census (tests/dispatch_census.py) -- every (call form, kernel, ksize,
stride, edge bits) combination the library's dispatch can pick over the accepted input space, run at its cheapest geometry through
the entry point the engine uses, against fp32 ATen on the GPU (TF32 off) on bf16-representable data.

Bars (those of test_train_ops_gpu.py / test_conv_gpu.py): bf16 outputs and data gradients 2 bf16 ulp of the contributing
magnitudes + 3e-3; weight gradients max error <= 2e-3 * max|ref| + 1e-3; batch statistics vs fp64 sums of the stored z at
rtol 1e-4 / atol 1e-2.  Every output buffer carries sentinels: the channels outside the launch's slice of a wider (route-concat)
buffer and a guard region past its end must come back bit-unchanged.

The fused YOLO head (conv + decode in one launch) is judged on its raw head values (p, against the reference conv) and its
decoded rows, which must equal the library's decode kernel applied to those head values bit for bit.  That second comparison is not
independent of the library: the decode arithmetic itself is held to the oracle's forward by test_model_gpu.py (the full-size cases
run the fused heads at 608^2, 512^2 and 416 x 640).

Weight gradients run both ways the library offers: ryolo_conv2d_wgrad (tile kernel + the layer's own split-K reduce) and, as the
training engine runs them, ryolo_conv2d_wgrad_partials followed by the batched reduce (ryolo_conv_wgrad_reduce_batch).
"""
import ctypes as C
import time

import pytest
import torch
import torch.nn.functional as F

from tests import dispatch_census as dc

pytestmark = pytest.mark.gpu

SENT = -777.0          # exactly representable in bf16
GUARD = 4096


@pytest.fixture(scope="module")
def env(cuda_dev):
    from rotate_yolov3_amd import _lib
    from rotate_yolov3_amd.model import hip_ops, hip_train_ops
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    cus = torch.cuda.get_device_properties(cuda_dev).multi_processor_count

    class NS:
        ops, tr, lib = hip_ops, hip_train_ops, _lib
    NS.cus = cus
    return NS


def _guarded(shape, cs, dev, fill=SENT):
    """an NHWC bf16 buffer [N, H, W, cs] followed by GUARD sentinel elements; returns (flat, full view)"""
    n, h, w = shape
    flat = torch.full((n * h * w * cs + GUARD,), fill, dtype=torch.bfloat16, device=dev)
    return flat, flat[:n * h * w * cs].view(n, h, w, cs)


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


def _check_sentinels(flat, full, off, c, what):
    torch.cuda.synchronize()
    assert bool((flat[full.numel():] == SENT).all()), "%s: store past the end of the buffer" % what
    if off > 0:
        assert bool((full[..., :off] == SENT).all()), "%s: store into the channels before the slice" % what
    if off + c < full.shape[-1]:
        assert bool((full[..., off + c:] == SENT).all()), "%s: store into the channels after the slice" % what


def _bar(got, want, mag, what, extra=3e-3):
    err = (got.double() - want.double()).abs()
    lim = 2 ** -7 * mag.double() + extra
    bad = err > lim
    assert not bool(bad.any()), "%s: %d of %d values off, worst err %.4g (limit there %.4g)" % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(lim.flatten()[int((err - lim).flatten().argmax())]))


def _nchw(t):
    return t.float().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _act(v, act, slope):
    return torch.where(v > 0, v, v * slope) if act == 1 else v


def _run_eval(E, r, g, dev):
    t = r["desc"]
    N, H, W, Cin, Cout, k, s, pad, in_cs, out_cs, res_cs, act, slope, ups = t[:14]
    Ho, Wo = dc._out_hw(t)
    x = _rand(g, N, H, W, in_cs).to(dev)
    wt = _rand(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5).to(dev)
    scale = (torch.rand(Cout, generator=g) + 0.5).to(dev)
    shift = (torch.randn(Cout, generator=g) * 0.3).to(dev)
    packed = E.ops.pack_weights(wt, cin_pad=Cin)
    cp = E.ops.cpad(Cout)
    sc, sh = E.ops.pad_vec(scale, cp), E.ops.pad_vec(shift, cp)
    off = r["out_off"]
    flat, full = _guarded((N, Ho * ups, Wo * ups), out_cs, dev)
    out = full[..., off:off + Cout]
    res = None
    if r["residual"]:
        res = _rand(g, N, Ho, Wo, res_cs).to(dev).to(torch.bfloat16)[..., :Cout]
    xb = x.to(torch.bfloat16)[..., :Cin]
    E.ops.conv2d_bn_act(xb, packed, sc, sh, Cout, k, s, pad, act, slope, residual=res, out=out, upsample=ups)
    z = F.conv2d(_nchw(xb), wt, None, s, pad)
    mag = F.conv2d(_nchw(xb).abs(), wt.abs(), None, s, pad) * scale.view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    want = _act(z * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), act, slope)
    if res is not None:
        want = want + _nchw(res)
        mag = mag + _nchw(res).abs()
    if ups == 2:
        want = want.repeat_interleave(2, 2).repeat_interleave(2, 3)
        mag = mag.repeat_interleave(2, 2).repeat_interleave(2, 3)
    _bar(_nchw(out), want, mag, "eval output")
    _check_sentinels(flat, full, off, Cout, "eval output")


def _run_pair(E, r, g, dev):
    a, b = r["descs"]
    N, H, W, Cin, C1, k1, s1, p1, in_cs = a[:9]
    C2, k2, s2, p2, out_cs = b[4], b[5], b[6], b[7], b[9]
    x = _rand(g, N, H, W, in_cs).to(dev).to(torch.bfloat16)[..., :Cin]
    w1 = _rand(g, C1, Cin, k1, k1, scale=(Cin * k1 * k1) ** -0.5).to(dev)
    w2 = _rand(g, C2, C1, k2, k2, scale=(C1 * k2 * k2) ** -0.5).to(dev)
    sc1, sh1 = (torch.rand(C1, generator=g) + 0.5).to(dev), (torch.randn(C1, generator=g) * 0.3).to(dev)
    sc2, sh2 = (torch.rand(C2, generator=g) + 0.5).to(dev), (torch.randn(C2, generator=g) * 0.3).to(dev)
    first = dict(cout=C1, ksize=k1, stride=s1, pad=p1, act=a[11], slope=a[12])
    second = dict(cout=C2, ksize=k2, stride=s2, pad=p2, act=b[11], slope=b[12])
    assert E.ops.conv_pair_supported(x, first, second, r["shortcut"])
    ho, wo = dc._out_hw(b)
    flat, full = _guarded((N, ho, wo), out_cs, dev)
    out = full[..., :C2]
    E.ops.conv2d_bn_act_pair(x, first, second, E.ops.pack_weights(w1, cin_pad=Cin), E.ops.pad_vec(sc1, E.ops.cpad(C1)),
                             E.ops.pad_vec(sh1, E.ops.cpad(C1)), E.ops.pack_weights(w2, cin_pad=C1), E.ops.pad_vec(sc2, E.ops.cpad(C2)),
                             E.ops.pad_vec(sh2, E.ops.cpad(C2)), shortcut_from_input=r["shortcut"], out=out)
    y1 = _act(F.conv2d(_nchw(x), w1, None, s1, p1) * sc1.view(1, -1, 1, 1) + sh1.view(1, -1, 1, 1), a[11], a[12])
    y1 = y1.to(torch.bfloat16).float()                     # the intermediate tensor lives in LDS as bf16
    want = _act(F.conv2d(y1, w2, None, s2, p2) * sc2.view(1, -1, 1, 1) + sh2.view(1, -1, 1, 1), b[11], b[12])
    mag = F.conv2d(y1.abs(), w2.abs(), None, s2, p2) * sc2.view(1, -1, 1, 1) + sh2.abs().view(1, -1, 1, 1)
    if r["shortcut"]:
        want, mag = want + _nchw(x), mag + _nchw(x).abs()
    _bar(_nchw(out), want, mag, "stem pair output")
    _check_sentinels(flat, full, 0, C2, "stem pair output")


def _run_head(E, r, g, dev):
    t = r["desc"]
    N, H, W, Cin, Cout = t[:5]
    in_cs = t[8]
    na, no = r["na"], r["no"]
    L = E.lib.lib()
    x = _rand(g, N, H, W, in_cs).to(dev).to(torch.bfloat16)
    wt = _rand(g, Cout, Cin, 1, 1, scale=Cin ** -0.5).to(dev)
    shift = (torch.randn(Cout, generator=g) * 0.3).to(dev)
    cp = E.ops.cpad(Cout)
    packed = E.ops.pack_weights(wt, cin_pad=Cin)
    sc, sh = E.ops.pad_vec(torch.ones(Cout, device=dev), cp), E.ops.pad_vec(shift, cp)
    anchors = torch.cat([torch.rand(na, 2, generator=g) * 40 + 4, (torch.rand(na, 1, generator=g) - 0.5) * 3], 1).to(dev).contiguous()
    rows = na * H * W
    io = torch.full((N, rows + 8, no), -5.0, dtype=torch.float32, device=dev)
    p = torch.full((N, na, H, W, no), -5.0, dtype=torch.float32, device=dev)
    d = dc.mk_desc(t)
    stride = 32.0
    E.lib.check(L.ryolo_conv_head_decode(C.byref(d), x.data_ptr(), packed.data_ptr(), sc.data_ptr(), sh.data_ptr(), anchors.data_ptr(), na,
                                         no, stride, 1.0, 0, io.data_ptr(), rows + 8, 4, p.data_ptr(), E.lib.stream_ptr(dev)),
                "ryolo_conv_head_decode")
    xin = _nchw(x[..., :Cin])
    z = F.conv2d(xin, wt) + shift.view(1, -1, 1, 1)
    mag = F.conv2d(xin.abs(), wt.abs()) + shift.abs().view(1, -1, 1, 1)
    pr = p.permute(0, 1, 4, 2, 3).reshape(N, na * no, H, W)        # [N, na, ny, nx, no] -> channel a * no + k
    _bar(pr, z, mag, "fused head values")
    head = p.permute(0, 2, 3, 1, 4).reshape(N, H, W, na * no).to(torch.bfloat16).contiguous()
    assert torch.equal(head.float(), p.permute(0, 2, 3, 1, 4).reshape(N, H, W, na * no)), "head values are not bf16"
    io2 = torch.full_like(io, -5.0)
    E.lib.check(L.ryolo_yolo_decode(head.data_ptr(), na * no, N, H, W, na, no, anchors.data_ptr(), stride, 1.0, 0, io2.data_ptr(), rows + 8, 4,
                                    None, E.lib.stream_ptr(dev)), "ryolo_yolo_decode")
    torch.cuda.synchronize()
    assert torch.equal(io, io2), float((io - io2).abs().max())
    assert bool((io[:, :4] == -5.0).all()) and bool((io[:, 4 + rows:] == -5.0).all()), "decode rows outside the head's row range"


def _run_train(E, r, g, dev):
    t = r["desc"]
    N, H, W, Cin, Cout, k, s, pad, in_cs = t[:9]
    Ho, Wo = dc._out_hw(t)
    tr = E.tr
    x = _rand(g, N, H, W, in_cs).to(dev).to(torch.bfloat16)
    if r["recompute"]:
        x[..., 3:] = 0                                        # layer 0: 3 real channels padded to 8
    xv = x[..., :Cin]
    wt = _rand(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5).to(dev)
    cp = E.ops.cpad(Cout)
    packed = E.ops.pack_weights(wt, cin_pad=Cin)
    ones = torch.ones(cp, device=dev)
    d = dc.mk_desc(t)
    flat, z = _guarded((N, Ho, Wo), Cout, dev)
    ref = F.conv2d(_nchw(xv), wt, None, s, pad)
    mag = F.conv2d(_nchw(xv).abs(), wt.abs(), None, s, pad)
    if not r["stats"]:
        bias = (torch.randn(Cout, generator=g) * 0.3).to(dev)
        tr.conv_fwd_plain(d, xv, packed, ones, E.ops.pad_vec(bias, cp), z)
        _bar(_nchw(z), ref + bias.view(1, -1, 1, 1), mag + bias.abs().view(1, -1, 1, 1), "training forward (bias conv)")
        _check_sentinels(flat, z, 0, Cout, "training forward")
        return
    zeros = torch.zeros(cp, device=dev)
    part = tr.conv_fwd_stats(d, xv, packed, ones, zeros, z)
    _bar(_nchw(z), ref, mag, "training forward z")
    _check_sentinels(flat, z, 0, Cout, "training forward z")
    z64 = z.double().view(-1, Cout)
    s1, s2 = part[:, 0, :Cout].sum(0), part[:, 1, :Cout].sum(0)
    assert torch.allclose(s1, z64.sum(0), rtol=1e-4, atol=1e-2), float((s1 - z64.sum(0)).abs().max())
    assert torch.allclose(s2, (z64 * z64).sum(0), rtol=1e-4, atol=1e-2), float((s2 - (z64 * z64).sum(0)).abs().max())
    if r["recompute"]:
        # layer 0 trains without storing z: the statistics-only pass must give the stored-z pass's sums, and the recomputing
        # BatchNorm + activation forward the activation of those statistics
        d2 = dc.mk_desc(t)
        part0 = tr.conv_fwd_stats(d2, xv, packed, ones, zeros, None)
        assert torch.allclose(part0.sum(0), part.sum(0), rtol=1e-12, atol=1e-9)
        gamma = (torch.rand(Cout, generator=g) + 0.5).to(dev)
        beta = (torch.randn(Cout, generator=g) * 0.3).to(dev)
        mean, invstd, scale, shift = tr.bn_finalize(part, Cout, N * Ho * Wo, gamma, beta)
        slope = torch.tensor([0.1], device=dev)
        flat_y, y = _guarded((N, Ho, Wo), Cout, dev)
        tr.conv0_bn_act_fwd(dc.mk_desc(t), xv, packed, scale, shift, 1, slope, y)
        want = _act(_nchw(z) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), 1, 0.1)
        mag_y = _nchw(z).abs() * scale.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
        _bar(_nchw(y), want, mag_y, "layer-0 recomputing forward", extra=1e-2)
        _check_sentinels(flat_y, y, 0, Cout, "layer-0 recomputing forward")


def _run_dgrad(E, r, g, dev, acc):
    t = r["desc"]
    N, H, W, Cin, Cout, k, s, pad, in_cs = t[:9]
    Ho, Wo = dc._out_hw(t)
    tr = E.tr
    wt = _rand(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5).to(dev)
    dz = _rand(g, N, Ho, Wo, Cout).to(dev).to(torch.bfloat16)
    pk = tr.pack_weights_dgrad(wt, s)
    cp = E.ops.cpad(Cin)
    ones, zeros = torch.ones(cp, device=dev), torch.zeros(cp, device=dev)
    prev = _rand(g, N, H, W, Cin).to(dev).to(torch.bfloat16)
    flat, full = _guarded((N, H, W), in_cs, dev)
    dx = full[..., :Cin]
    if acc:
        dx.copy_(prev)
    d = dc.mk_desc(t)
    z = stats = part = slope = None
    if r["bnred"]:
        z = (_rand(g, N, H, W, Cin) * 1.5).to(dev).to(torch.bfloat16)
        zf = z.float().view(-1, Cin)
        gamma, beta = (torch.rand(Cin, generator=g) + 0.5).to(dev), (torch.randn(Cin, generator=g) * 0.3).to(dev)
        mean, invstd = zf.mean(0), (zf.var(0, unbiased=False) + 1e-5).rsqrt()
        scale = gamma * invstd
        stats = (mean.contiguous(), invstd.contiguous(), scale.contiguous(), (beta - mean * scale).contiguous())
        slope = torch.tensor([0.1], device=dev)
        rows = tr.dgrad_bnreduce_rows(d)
        assert rows > 0
        part = torch.full((rows, 3, Cin), 123.0, device=dev)
        tr.conv_dgrad_bnreduce(d, dz, pk, ones, zeros, dx, acc, z, stats, slope, part)
    else:
        tr.conv_dgrad(d, dz, pk, ones, zeros, dx, acc)
    gx = torch.nn.grad.conv2d_input((N, Cin, H, W), wt, _nchw(dz), s, pad)
    mag = torch.nn.grad.conv2d_input((N, Cin, H, W), wt.abs(), _nchw(dz).abs(), s, pad)
    if acc:
        gx, mag = gx + _nchw(prev), mag + _nchw(prev).abs()
    _bar(_nchw(dx), gx, mag, "data gradient (accumulate %d)" % acc)
    _check_sentinels(flat, full, 0, Cin, "data gradient")
    if r["bnred"]:
        M = N * H * W
        ws = torch.empty(tr.bn_bwd_ws_bytes(M, Cin), dtype=torch.uint8, device=dev)
        dzb = torch.empty_like(z)
        dg, db, ds = torch.zeros(Cin, device=dev), torch.zeros(Cin, device=dev), torch.zeros(1, device=dev)
        tr.bn_act_bwd_reduced(z, dx.contiguous() if in_cs != Cin else dx, stats, 1, slope, dzb, dg, db, ds, part, ws)
        torch.cuda.synchronize()
        d64, z64 = dx.double().reshape(-1, Cin), z.double().view(-1, Cin)
        u = z64 * stats[2].double() + stats[3].double()
        gg = torch.where(u > 0, d64, d64 * 0.1)
        assert torch.allclose(db.double(), gg.sum(0), rtol=1e-4, atol=1e-2), float((db.double() - gg.sum(0)).abs().max())
        assert torch.allclose(dg.double(), (gg * (z64 - stats[0].double()) * stats[1].double()).sum(0), rtol=1e-4, atol=1e-2)


def _run_wgrad(E, r, g, dev):
    t = r["desc"]
    N, H, W, Cin, Cout, k, s, pad, in_cs = t[:9]
    Ho, Wo = dc._out_hw(t)
    tr = E.tr
    x = _rand(g, N, H, W, in_cs).to(dev).to(torch.bfloat16)
    xv = x[..., :Cin]
    dz = _rand(g, N, Ho, Wo, Cout).to(dev).to(torch.bfloat16)
    d = dc.mk_desc(t)
    ws = torch.empty(tr.wgrad_ws_bytes(d), dtype=torch.uint8, device=dev)
    grad = torch.full((Cout, Cin, k, k), 0.5, device=dev)
    tr.conv_wgrad(d, xv, dz, r["cin_real"], grad, True, ws)
    # the training engine's form: partial tiles into the layer's own workspace, then the batched split-K reduce
    ws_b = torch.empty(max(tr.wgrad_ws_bytes(d), 256), dtype=torch.uint8, device=dev)
    grad_b = torch.full((Cout, Cin, k, k), 0.5, device=dev)
    tr.conv_wgrad_partials(d, xv, dz, r["cin_real"], grad_b, True, ws_b)
    wb = tr.WgradReduceBatch(dev)
    wb.add(d, r["cin_real"], ws_b, grad_b, True)
    wb.finalize()
    wb.run()
    ref = torch.nn.grad.conv2d_weight(_nchw(xv), (Cout, Cin, k, k), _nchw(dz), s, pad)
    torch.cuda.synchronize()
    lim = 2e-3 * float(ref.abs().max()) + 1e-3
    for what, gw in (("weight gradient", grad), ("weight gradient, batched reduce", grad_b)):
        err = float((gw - 0.5 - ref).abs().max())
        assert err <= lim, (what, err, lim)


def _kernel_of(E, r):
    """the kernel-choice call on the representative's descriptor (must give the class's kernel)"""
    L = E.lib.lib()
    if r["form"] == "eval":
        return L.ryolo_conv_kernel_choice(C.byref(dc.mk_desc(r["desc"])), 1 if r["residual"] else 0, 0)
    if r["form"] == "train":
        return L.ryolo_conv_kernel_choice(C.byref(dc.mk_desc(r["desc"])), 0, 1 if r["stats"] else 0)
    if r["form"] == "dgrad":
        return L.ryolo_conv_dgrad_kernel_choice(C.byref(dc.mk_desc(r["desc"])), 1 if r["bnred"] else 0)
    if r["form"] == "wgrad":
        return L.ryolo_conv_wgrad_kernel_choice(C.byref(dc.mk_desc(r["desc"])))
    if r["form"] == "pair":
        a, b = r["descs"]
        return 1 if L.ryolo_conv_pair_supported(C.byref(dc.mk_desc(a)), C.byref(dc.mk_desc(b)), 1 if r["shortcut"] else 0) else -1
    return 1 if L.ryolo_conv_head_decode_supported(C.byref(dc.mk_desc(r["desc"])), r["na"], r["no"]) else -1


def test_every_census_class_against_aten(env, cuda_dev):
    t0 = time.time()
    refused = []
    classes = dc.census(cus=env.cus, refused=refused)
    print("\ndispatch census on %d CUs: %d edge classes; %d (config, size, batch) points refused by the engines (%s)" % (
        env.cus, len(classes), len(refused), sorted(set(e for _, e in refused))))
    print(dc.format_table(classes))
    checked = 0
    for n, key in enumerate(sorted(classes, key=str)):
        r = classes[key]["rep"]
        assert _kernel_of(env, r) == r["code"], (key, r["point"])
        g = torch.Generator().manual_seed(1000 + n)
        what = "%s at %s layer %d" % (key[:4], r["point"], r["layer"])
        try:
            form = r["form"]
            if form == "eval":
                _run_eval(env, r, g, cuda_dev)
            elif form == "pair":
                _run_pair(env, r, g, cuda_dev)
            elif form == "head":
                _run_head(env, r, g, cuda_dev)
            elif form == "train":
                _run_train(env, r, g, cuda_dev)
            elif form == "dgrad":
                _run_dgrad(env, r, g, cuda_dev, False)
                _run_dgrad(env, r, g, cuda_dev, True)
            elif form == "wgrad":
                _run_wgrad(env, r, g, cuda_dev)
            else:
                raise KeyError(form)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e))
        checked += 1
        torch.cuda.empty_cache()
    print("checked %d of %d classes in %.1f s" % (checked, len(classes), time.time() - t0))
    assert checked == len(classes)


def test_census_matches_the_engines(env, cuda_dev):
    """the census plans from the cfg text, the engines from the modules (same planner, model/plan.py), pinned at 608^2 / bs 4: every training
    block's descriptor equals the engine's block's desc field by field, the inference engine's conv launches (layer, kernel name) equal
    the census's, and the tensors the engine materialised have the plan's geometry"""
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.model.engine import HipEngine
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.model.train_engine import TrainEngine
    shape = (4, 3, 608, 608)
    m = Darknet(make_cfg.darknet53(608, 608), {"context_factor": 1.0}).to(cuda_dev)
    defs = dc.config_defs("darknet53", 1, 608, 608)
    te = TrainEngine(m, shape, cuda_dev)
    recs = dc.train_blocks(defs, 608, 608, 4)
    want = {r["layer"]: r for r in recs if r["form"] == "train"}
    assert sorted(want) == [b.i for b in te.blocks]
    for b in te.blocks:
        assert dc.desc_tuple(b.desc) == dc.desc_tuple(dc.mk_desc(want[b.i]["desc"])), (b.i, dc.desc_tuple(b.desc))
        assert b.recompute == want[b.i]["recompute"]
    te._plan_reduce_fusion()                                 # (static: needs no forward)
    red = {r["layer"]: r["bnred"] for r in recs if r["form"] == "dgrad"}
    assert {b.i: b.red_for is not None for b in te.blocks if b.xin_g is not None} == red
    assert sorted(r["layer"] for r in recs if r["form"] == "wgrad") == [b.i for b in te.blocks if b.has_wgrad]
    del te
    torch.cuda.empty_cache()
    he = HipEngine(m.eval(), shape, cuda_dev)
    got = sorted((o["layer"], o["name"]) for o in he.op_info if o["kind"] == "conv")
    erecs = dc.eval_blocks(defs, 608, 608, 4)
    mine = sorted((r["layer"], r["name"]) for r in erecs)
    assert got == mine
    # the geometry the eval parity cases are built from: input / output / residual pixel strides, the output's channel offset inside a
    # route-concat buffer (the engine's buffers are allocated whole, so a view's storage offset is its channel offset), spatial shape
    nchk = 0
    for r in erecs:
        if r["form"] != "eval":
            continue
        i, t = r["layer"], r["desc"]
        xin = he.x_nhwc if i == 0 else he.views[i - 1]
        out = he.views[i]
        assert (xin.shape[0], xin.shape[1], xin.shape[2], xin.shape[3], xin.stride(2)) == (t[0], t[1], t[2], t[3], t[8]), (i, t)
        assert out.stride(2) == t[9] and out.storage_offset() == r["out_off"] and out.shape[3] == t[4], (i, t, out.storage_offset())
        if r["residual"]:
            assert he.views[r["res_layer"]].stride(2) == t[10], (i, t)
        nchk += 1
    assert nchk == sum(r["form"] == "eval" for r in erecs) and nchk > 0
    del he
    torch.cuda.empty_cache()
