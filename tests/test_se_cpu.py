"""CPU tier of the squeeze-and-excitation layers: cfg / module / state dict against the reference's goldens, the ATen chain, the
bf16 emulation (tests/se_reference.py) against the pinned oracle, the planner's se ops and refusals, the C ABI's host-side checks."""
import ctypes as C
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from oracle import darknet_oracle as do
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import plan
from rotate_yolov3_amd.model.models import Darknet, SELayer
from rotate_yolov3_amd.utils.parse_config import parse_model_cfg_text
from tests import dispatch_census as dc
from tests import se_reference as sr
from tests.procedural import fill_procedural

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SE_LAYERS = list(range(13, 42, 4)) + list(range(46, 75, 4)) + list(range(79, 92, 4))


def _se_model(size=64):
    cfg = make_cfg.darknet53_se(size, size)
    return cfg, sr.fill_se(fill_procedural(Darknet(cfg, {"context_factor": 1.0}).eval()))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "forward_d53se_64.npz"))


def test_make_cfg_darknet53_se_is_the_reference_topology():
    ref = json.load(open(os.path.join(G, "parser_ref_cfgs.json")))["cfgs"]["cfg/ICDAR/yolov3_608_se.cfg"]["blocks"][1:]
    got = parse_model_cfg_text(make_cfg.darknet53_se(608, 608))[1:]
    assert len(got) == len(ref) == 127
    assert [i for i, d in enumerate(got) if d["type"] == "se"] == SE_LAYERS
    for i, (a, b) in enumerate(zip(got, ref)):
        kv = dict(b["kv"])
        assert a["type"] == b["type"], i
        for key in ("filters", "size", "stride", "channels", "from", "layers"):
            if key in kv or key in a:
                assert str(a[key]).strip() == kv[key].strip(), (i, key)
    # and the plain generator did not move: no se block, from=-3 everywhere
    plain = parse_model_cfg_text(make_cfg.darknet53(608, 608))[1:]
    assert len(plain) == 107 and all(d["from"] == "-3" for d in plain if d["type"] == "shortcut")


def test_state_dict_keys_and_loading(golden):
    cfg, m = _se_model()
    keys = [str(k) for k in golden["keys"]]
    assert list(m.state_dict().keys()) == keys
    assert sum(k.endswith("fc.0.weight") for k in keys) == 20 and "module_list.13.fc.2.weight" in keys
    assert isinstance(m.module_list[13], SELayer) and m.module_list[13].fc[0].weight.shape == (16, 256)
    fresh = Darknet(cfg, {"context_factor": 1.0})
    fresh.load_state_dict({k: m.state_dict()[k].clone() for k in keys}, strict=True)
    assert torch.equal(fresh.module_list[91].fc[2].weight, m.module_list[91].fc[2].weight)


def test_cpu_forward_equals_the_reference_golden(golden):
    cfg, m = _se_model()
    x = torch.from_numpy(golden["x"])
    gates = {}
    for i in SE_LAYERS:
        m.module_list[i].fc.register_forward_hook(lambda mod, inp, out, i=i: gates.__setitem__(i, out.reshape(-1)))
    with torch.no_grad():
        io, p = m(x)
    assert np.allclose(io.numpy(), golden["io"], rtol=1e-5, atol=1e-5), np.abs(io.numpy() - golden["io"]).max()
    for k in range(3):
        assert np.allclose(p[k].numpy(), golden["p%d" % k], rtol=1e-5, atol=1e-5)
    for i in SE_LAYERS:
        g = golden["gate_%d" % i]
        assert np.allclose(gates[i].numpy(), g, rtol=1e-5, atol=1e-6)
        assert g.min() < 0.35 and g.max() > 0.65          # the fixture's gates are far from the trivial 0.5
    # the fp32 emulation is the same operator chain again
    io_e, p_e, gates_e = sr.forward(cfg, m.state_dict(), x, return_gates=True)
    assert np.allclose(io_e.numpy(), golden["io"], rtol=2e-4, atol=2e-4)
    assert all(np.allclose(a.reshape(-1).numpy(), golden["gate_%d" % i], rtol=1e-4, atol=1e-5) for a, i in zip(gates_e, SE_LAYERS))


def bf16_emulation_error_vs_golden():
    """(max rel, mean rel) error, in the terms of tests/test_model_gpu._cmp, of se_reference.forward(bf16=True) against the reference's
    fp32 golden: the GPU tier allows the engine twice this"""
    z = np.load(os.path.join(G, "forward_d53se_64.npz"))
    cfg, m = _se_model()
    io_b, _ = sr.forward(cfg, m.state_dict(), torch.from_numpy(z["x"]), bf16=True)
    want = torch.from_numpy(z["io"])
    scale = want.abs().mean().item() + 1e-6
    err = (io_b - want).abs()
    return (err / (want.abs() + scale)).max().item(), err.mean().item() / scale


def test_bf16_emulation_stays_near_the_fp32_golden():
    e_max, e_mean = bf16_emulation_error_vs_golden()
    print("se_reference.forward(bf16=True) vs the reference's fp32 golden: max rel %.4g  mean rel %.4g" % (e_max, e_mean))
    assert e_max < 0.05 and e_mean < 0.01                 # bf16-level agreement (three-digit mantissa through 75 conv layers)


def test_emulation_equals_the_pinned_oracle_on_a_plain_cfg():
    cfg = make_cfg.darknet53(64, 64)
    m = fill_procedural(Darknet(cfg, {"context_factor": 1.0}).eval())
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    io_o, p_o = do.forward(cfg, m.state_dict(), x, bf16=True)
    io_e, p_e = sr.forward(cfg, m.state_dict(), x, bf16=True)
    assert torch.equal(io_o, io_e) and all(torch.equal(a, b) for a, b in zip(p_o, p_e))


def _plan(cfg_text, N, H, W, **kw):
    defs = parse_model_cfg_text(cfg_text)[1:]
    return defs, plan.plan_eval(defs, dc._convs(defs), dc._yolos(defs), N, H, W, **kw)


def test_plan_eval_of_the_se_cfg():
    defs, pl = _plan(make_cfg.darknet53_se(608, 608), 32, 608, 608)
    se = [op for op in pl.ops if op["kind"] == "se"]
    assert [op["layer"] for op in se] == SE_LAYERS
    assert [op["C"] for op in se] == [256] * 8 + [512] * 8 + [1024] * 4
    for op in se:
        assert op["out"] != op["xin"] and op["out"].buf != op["xin"].buf and op["xin"] == pl.views[op["layer"] - 1]
        assert (op["out"].H, op["out"].W) == {256: (76, 76), 512: (38, 38), 1024: (19, 19)}[op["C"]]
    _, plain = _plan(make_cfg.darknet53(608, 608), 32, 608, 608)
    fam = ("conv", "pair", "head")
    assert sum(op["kind"] in fam for op in pl.ops) == sum(op["kind"] in fam for op in plain.ops)
    # the conv in front of an se still folds its shortcut; nothing but conv-family, se and decode launches
    assert not [op for op in pl.ops if op["kind"] in ("add", "upsample", "copy", "maxpool")]
    res = [op for op in pl.ops if op["kind"] == "conv" and op["res"] is not None]
    assert len([op for op in res if defs[op["layer"] - 2]["type"] == "se"]) == 20
    for op in res:
        if defs[op["layer"] - 2]["type"] == "se":
            assert op["res"] == pl.views[op["layer"] - 3]            # the skip is the se's INPUT
    # the stem-pair and head rules never reach across an se
    for op in pl.ops:
        if op["kind"] == "pair":
            assert op["layer"] - op["first"] == 1 and defs[op["first"]]["type"] == "convolutional"


def test_plan_eval_of_an_se_that_is_a_route_source_writes_its_home_slice():
    cfg = "\n".join(["[net]", "width=64", "height=64", "channels=3", ""]
                    + make_cfg._conv(32, 3, 1) + ["[se]", "channels=32", ""] + make_cfg._conv(16, 1, 1)
                    + ["[route]", "layers = -1, -2", ""] + make_cfg._conv(56, 1, 1, bn=0, act="linear")
                    + make_cfg._yolo("0-7", "ara 100, 200 / 2 / 0, 30, 60, 90", 1)) + "\n"
    defs, pl = _plan(cfg, 2, 64, 64)
    se = [op for op in pl.ops if op["kind"] == "se"][0]
    assert se["out"].buf == pl.views[3].buf and (se["out"].off, se["out"].C, se["out"].cs) == (16, 32, 48)
    assert not [op for op in pl.ops if op["kind"] == "copy"]


def test_plan_eval_refuses_se_widths_the_kernels_do_not_serve():
    for c in (8,):        # (a width that is no multiple of 8 is refused by the conv in front of it already)
        cfg = "\n".join(["[net]", "width=64", "height=64", "channels=3", ""] + make_cfg._conv(c, 3, 1) + ["[se]", "channels=%d" % c, ""]
                        + make_cfg._conv(56, 1, 1, bn=0, act="linear") + make_cfg._yolo("0-7", "ara 100, 200 / 2 / 0, 30, 60, 90", 1)) + "\n"
        with pytest.raises(plan.Refused, match=r"^se 1: 8 channels"):
            _plan(cfg, 1, 64, 64)


# launches per kind of the plain Darknet-53 plan at 608^2 with the library's fusions off (no device query: the same on every machine),
# counted on the parent of the commit that added the se op
PLAIN_KINDS = {"conv": 75, "decode": 3}


def test_plan_eval_of_the_plain_cfg_did_not_move():
    defs, pl = _plan(make_cfg.darknet53(608, 608), 32, 608, 608, stem_pair=False, head_decode=False)
    assert dict(Counter(op["kind"] for op in pl.ops)) == PLAIN_KINDS
    convs = [op for op in pl.ops if op["kind"] == "conv"]
    assert sum(op["res"] is not None for op in convs) == 23 and sum(op["ups"] == 2 for op in convs) == 2
    assert len(pl.buffers) == 74                        # the input, 2 concat buffers, 71 conv outputs (23 shortcuts and 2 upsamples folded, 4 homed)
    for op in convs:                                    # descriptors: (N, H, W, Cin, Cout, k, s, pad, in_cs, out_cs, res_cs, act, slope, ups, tile)
        d, cv = op["desc"], dc._convs(defs)[op["layer"]]
        assert d[0] == 32 and d[4:8] == (cv["cout"], cv["k"], cv["s"], cv["pad"]) and d[8] == op["xin"].cs and d[9] == op["out"].cs
    _, pl2 = _plan(make_cfg.darknet53(608, 608), 32, 608, 608)
    assert set(op["kind"] for op in pl2.ops) <= {"conv", "pair", "head", "decode"}
    assert sum({"pair": 2, "head": 2}.get(op["kind"], 1) for op in pl2.ops) == 78


def test_plan_train_refuses_se():
    defs = parse_model_cfg_text(make_cfg.darknet53_se(96, 96))[1:]
    with pytest.raises(plan.Refused, match=r"se layers have no HIP training kernels \(use model.backend = 'torch'\)"):
        plan.plan_train(defs, dc._convs(defs), 2, 96, 96)


def test_torch_backend_trains_one_cpu_step():
    from rotate_yolov3_amd.model.loss import compute_loss
    z = np.load(os.path.join(G, "loss_d53_96.npz"))
    hyp = {k: float(v) for k, v in zip(z["hyp_keys"], z["hyp_vals"])}
    cfg = make_cfg.darknet53_se(64, 64)
    m = sr.fill_se(fill_procedural(Darknet(cfg, hyp)))
    m.backend = "torch"
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    targets = torch.tensor([[0, 0, 0.5, 0.5, 0.3, 0.1, 0.2], [1, 0, 0.3, 0.6, 0.2, 0.2, -0.5]])
    p = m(x)
    assert len(p) == 3 and p[0].shape == (2, 72, 2, 2, 7)
    loss, _ = compute_loss(p, targets, m, hyp)
    loss.backward()
    w = m.module_list[13].fc[0].weight
    before = w.detach().clone()
    assert w.grad is not None and torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0
    assert all(torch.isfinite(q.grad).all() for q in m.parameters() if q.grad is not None)
    opt.step()
    assert not torch.equal(before, w.detach())


def test_fuse_keeps_the_eval_output():
    cfg, m = _se_model()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        io0, p0 = m(x)
        m.fuse()
        io1, p1 = m(x)
    assert isinstance(m.module_list[13], SELayer) and not any(isinstance(q, torch.nn.BatchNorm2d) for q in m.modules())
    for a, b in zip(p0, p1):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), float((a - b).abs().max())
    assert torch.allclose(io0, io1, rtol=1e-3, atol=1e-3)


def test_unsupported_layer_message_names_what_is_still_out_of_scope():
    cfg = make_cfg.darknet53(64, 64).replace("[upsample]", "[d-convolutional]", 1)
    with pytest.raises(ValueError) as e:
        Darknet(cfg)
    assert "d-convolutional / weight_from" in str(e.value) and "se /" not in str(e.value)


def test_unit_recipe_spreads_the_gates():
    x, w1, w2 = sr.unit_inputs(2, 8, 8, 256)
    _, g = sr.se_fp64(x, w1, w2)
    assert 0.1 < float((g < 0.25).double().mean()) and 0.1 < float((g > 0.75).double().mean())
    y32, g32 = sr.se_aten_fp32(x, w1, w2)
    y64, _ = sr.se_fp64(x, w1, w2)
    d = sr.bf16_ulp_diff(y32.to(torch.bfloat16), y64.to(torch.bfloat16))
    assert int(d.max()) <= 1 and float((d > 0).double().mean()) < 0.005
    assert float((g32.double() - g).abs().max()) < 1e-6


def _lib():
    from rotate_yolov3_amd import _lib as L
    return L.lib()


def test_se_abi_host_side_checks():
    lib = _lib()
    assert lib.ryolo_abi_version() == 4
    ws = lib.ryolo_se_workspace_bytes
    sizes = [ws(n, 76, 76, 256) for n in (1, 2, 3, 8, 32)]
    assert all(a > 0 for a in sizes) and all(a < b for a, b in zip(sizes[:-1], sizes[1:]))
    assert ws(32, 76, 76, 256) >= 32 * 256 * 4 * 2 and ws(1, 1, 1, 16) > 0
    assert ws(1, 8, 8, 12) == 0 and ws(1, 8, 8, 4096) == 0 and ws(0, 8, 8, 64) == 0 and ws(1, 8, 8, 8) == 0
    # argument checks return before anything is enqueued: no GPU needed, the pointers are never dereferenced
    x, y, w1, w2, wsp = (C.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20))
    big = C.c_size_t(1 << 30)

    def call(x=x, xcs=256, w1=w1, w2=w2, hidden=16, y=y, ycs=256, N=1, H=8, W=8, Cc=256, wsp=wsp, nbytes=big):
        return lib.ryolo_se_nhwc(x, xcs, w1, w2, hidden, y, ycs, N, H, W, Cc, None, wsp, nbytes, None)
    assert call(Cc=12, xcs=16, ycs=16) == -1
    assert call(Cc=4096, xcs=4096, ycs=4096) == -1
    assert call(hidden=0) == -1 and call(hidden=129) == -1
    assert call(x=None) == -1 and call(y=None) == -1 and call(w1=None) == -1 and call(w2=None) == -1 and call(wsp=None) == -1
    assert call(nbytes=C.c_size_t(ws(1, 8, 8, 256) - 1)) == -1
    assert call(xcs=248) == -1 and call(ycs=260) == -1 and call(x=C.c_void_p((1 << 20) + 8)) == -1
    assert call(y=x) == -1 and call(y=C.c_void_p((1 << 20) + 64)) == -1        # y overlapping x
    assert len(__import__("rotate_yolov3_amd")._lib.TUNING_SWITCHES) == 6
