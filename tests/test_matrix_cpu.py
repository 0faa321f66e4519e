"""CPU tier of the matrix cfgs (shared-weight `weight_from` layers, dilated `d-convolutional` layers): cfg / modules / state dict and the
ATen chain against the reference's golden, the shipped matrix cfgs, training through autograd, construction-time validation, the planner's
ops for them and its refusals, the host-side checks of ryolo_conv2d_dilated."""
import ctypes as C
import os
import shutil
from collections import Counter

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from oracle import darknet_oracle as do
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model import plan
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.utils.parse_config import parse_model_cfg_text
from tests import dispatch_census as dc
from tests import matrix_reference as mr
from tests.golden.gen_model_golden import REF
from tests.procedural import fill_procedural

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOURCES = list(range(75, 82)) + list(range(87, 94)) + list(range(99, 106))


def _matrix_model(size=96, na=8):
    cfg = make_cfg.darknet53_matrix(size, size, na_per_head=na)
    return cfg, mr.fill_matrix(fill_procedural(Darknet(cfg, {"context_factor": 1.0}).eval()))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "forward_matrix_96.npz"))


@pytest.fixture(scope="module")
def model96():
    return _matrix_model()


def test_make_cfg_darknet53_matrix_topology():
    defs = parse_model_cfg_text(make_cfg.darknet53_matrix(512, 512))[1:]
    kinds = Counter(d["type"] for d in defs)
    assert len(defs) == 244 and kinds["yolo"] == 16 and kinds["d-convolutional"] == 36
    assert sum(1 for d in defs if d["type"] == "convolutional" and "weight_from" in d) == 48
    assert mr.shared_sources(defs) == SOURCES
    assert [defs[i]["layers"].strip() for i in (107, 112, 123, 134)] == ["79", "74", "74", "86"]
    assert Counter(d["dilation"] for d in defs if d["type"] == "d-convolutional") == {
        "(1,2)": 9, "(2,1)": 9, "(1,4)": 6, "(4,1)": 6, "(1,8)": 3, "(8,1)": 3}
    # layers 0-106 are the plain generator's
    plain = parse_model_cfg_text(make_cfg.darknet53(512, 512))[1:]
    assert all({k: str(v) for k, v in a.items() if k != "anchors"} == {k: str(v) for k, v in b.items() if k != "anchors"}
               for a, b in zip(defs[:107], plain))


def test_state_dict_keys_equal_the_reference(golden, model96):
    cfg, m = model96
    keys = [str(k) for k in golden["keys"]]
    assert list(m.state_dict().keys()) == keys
    # a d-convolutional sharer owns BatchNorm buffers and no conv weight; a convolutional sharer owns a full (unused) block
    assert "module_list.114.BatchNorm2d.weight" in keys and "module_list.114.Conv2d.weight" not in keys
    assert "module_list.113.Conv2d.weight" in keys and "module_list.113.activation.weight" in keys
    assert isinstance(m.module_list[114].activation, torch.nn.LeakyReLU) and len(m.module_list[114].Conv2d) == 0


def test_cpu_forward_equals_the_reference_golden(golden, model96):
    cfg, m = model96
    x = torch.from_numpy(golden["x"])
    with torch.no_grad():
        io, p = m(x)
    assert len(p) == 16
    assert np.allclose(io.numpy(), golden["io"], rtol=1e-5, atol=1e-5), np.abs(io.numpy() - golden["io"]).max()
    for k in range(4):
        assert np.allclose(p[k].numpy(), golden["p%d" % k], rtol=1e-5, atol=1e-5)
    means = [float(q.abs().mean()) for q in p]
    assert np.allclose(means, golden["p_mean"], rtol=1e-4) and min(means[4:]) >= 0.1      # the matrix heads are far above any absolute floor
    # the fp32 emulation is the same operator chain again
    io_e, p_e = mr.forward(cfg, m.state_dict(), x)
    assert np.allclose(io_e.numpy(), golden["io"], rtol=2e-4, atol=2e-4)


FPN_ROWS = 8 * (9 + 36 + 144 + 4)      # rows of io that belong to the three FPN heads and the stride-64 head (written first)


def bf16_emulation_error_vs_golden(rows=slice(None)):
    """(max rel, mean rel) error, in the terms of tests/test_model_gpu._cmp, of matrix_reference.forward(bf16=True) against the reference's
    fp32 golden, over the given rows of io: the GPU tier allows the engine twice this"""
    z = np.load(os.path.join(G, "forward_matrix_96.npz"))
    cfg, m = _matrix_model()
    io_b, _ = mr.forward(cfg, m.state_dict(), torch.from_numpy(z["x"]), bf16=True)
    io_b, want = io_b[:, rows], torch.from_numpy(z["io"])[:, rows]
    scale = want.abs().mean().item() + 1e-6
    err = (io_b - want).abs()
    return (err / (want.abs() + scale)).max().item(), err.mean().item() / scale


def test_bf16_emulation_stays_near_the_fp32_golden():
    """The FPN and stride-64 heads keep bf16-level agreement with the fp32 golden.  The matrix heads are looser, and the reason is the
    trunk, not the branches: under fill_procedural its feature maps at layers 61 / 74 / 86 differ by 17 % / 8 % / 12 % (mean rel) between
    the bf16 and the fp32 forward, which the FPN heads' single-frequency filters do not see and the full-rank shared filters of
    tests/matrix_reference.fill_matrix pass on at gain 1.  Measured, bf16 emulation against the fp32 chain, mean rel per head: FPN 0.004 /
    0.024 / 0.004, stride-64 0.002, level 74: 0.074 / 0.106, level 86: 0.108 .. 0.114, level 98: 0.011 .. 0.012; whole io: max rel 0.168,
    mean rel 0.0196.  The model-level GPU bars of the matrix heads follow the CPU-measured sensitivity by the rule of
    tests/test_conv_dil_gpu._bars; what holds every dilated launch of the model to the conv tolerance is the per-launch test there."""
    e_max, e_mean = bf16_emulation_error_vs_golden(slice(0, FPN_ROWS))
    print("FPN + stride-64 rows: bf16 emulation vs the reference's fp32 golden: max rel %.4g  mean rel %.4g" % (e_max, e_mean))
    assert e_max < 0.05 and e_mean < 0.01                 # the bars of the se fixture
    a_max, a_mean = bf16_emulation_error_vs_golden()
    print("all rows: max rel %.4g  mean rel %.4g" % (a_max, a_mean))
    assert np.isfinite(a_max) and np.isfinite(a_mean)


def test_emulation_equals_the_pinned_oracle_on_a_plain_cfg():
    cfg = make_cfg.darknet53(64, 64)
    m = fill_procedural(Darknet(cfg, {"context_factor": 1.0}).eval())
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    io_o, p_o = do.forward(cfg, m.state_dict(), x, bf16=True)
    io_e, p_e = mr.forward(cfg, m.state_dict(), x, bf16=True)
    assert torch.equal(io_o, io_e) and all(torch.equal(a, b) for a, b in zip(p_o, p_e))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's cfg files are not on this machine")
@pytest.mark.parametrize("rel", ["cfg/HRSC+/yolov3_512_matrix.cfg", "cfg/yolov3-m.cfg", "cfg/HRSC/yolov3-m.cfg"])
def test_the_shipped_matrix_cfgs_construct(tmp_path, rel):
    path = str(tmp_path / os.path.basename(rel))
    shutil.copy(os.path.join(REF, rel), path)
    # utils/kmeans/anchor-cluster.txt is not in the reference: 18 (w, h) rows x 12 angles = the 216 anchors the masks index
    with open(str(tmp_path / "anchor-cluster.txt"), "w") as fh:
        fh.write("".join("%d %d\n" % (20 + 9 * i, 12 + 5 * i) for i in range(18)))
    m = Darknet(path, {"context_factor": 1.0})
    kinds = Counter(d["type"] for d in m.module_defs)
    assert kinds["yolo"] == 16 and kinds["d-convolutional"] == 36 and len(m.yolo_layers) == 16
    assert all("weight_from" in d for d in m.module_defs if d["type"] == "d-convolutional")


def test_aten_training_reaches_the_shared_weights_only():
    cfg, m = _matrix_model()
    m.train()
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(3))
    p = m(x)
    assert len(p) == 16 and all(q.requires_grad for q in p)
    sum(q.sum() for q in p).backward()
    for s in SOURCES:
        g = m.module_list[s].Conv2d.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, s
    sharers = [i for i, d in enumerate(m.module_defs) if "weight_from" in d]
    assert len(sharers) == 84
    for i in sharers:
        own = list(m.module_list[i].parameters())
        assert own and all(q.grad is None for q in own), i


def _edit(cfg, layer, **kv):
    """cfg text with keys of block `layer` (0 = the first block behind [net]) replaced"""
    out, k = [], -2
    for line in cfg.split("\n"):
        if line.startswith("["):
            k += 1
        key = line.split("=")[0].strip()
        out.append("%s=%s" % (key, kv[key]) if k == layer and key in kv else line)
    return "\n".join(out)


def test_weight_from_is_validated_at_construction():
    cfg = make_cfg.darknet53_matrix(96, 96, na_per_head=8)
    Darknet(cfg)
    for layer, kv, what in ((113, dict(weight_from="74"), "layer 113"),            # a shortcut layer
                            (125, dict(weight_from="113"), "layer 125"),           # a layer that shares a weight itself
                            (113, dict(weight_from="76"), "layer 113"),            # 3x3 1024 <- 512 weight for a 1x1 512 <- 1024 layer
                            (114, dict(filters="512"), "layer 114"),               # output channels
                            (114, dict(weight_from="88"), "layer 114"),            # input channels (256 -> 512 weight, 512 incoming)
                            (113, dict(weight_from="120"), "layer 113")):          # a later layer
        with pytest.raises(ValueError, match=what):
            Darknet(_edit(cfg, layer, **kv))
    # a d-convolutional block without weight_from has no weights in the reference either: the wording of before
    lines = cfg.split("\n")
    lines.pop(lines.index("weight_from = 76"))            # layer 114, the first d-convolutional block
    lone = "\n".join(lines)
    with pytest.raises(ValueError, match="d-convolutional / weight_from"):
        Darknet(lone)
    with pytest.raises(ValueError, match="dilation"):
        Darknet(_edit(cfg, 114, dilation="(0,2)"))


def test_multi_digit_dilations_parse():
    from rotate_yolov3_amd.model.models import parse_dilation
    assert parse_dilation({"dilation": "(1,2)"}) == (1, 2) and parse_dilation({"dilation": "(12, 3)"}) == (12, 3)


def test_fuse_raises_on_a_matrix_model(model96):
    cfg, m = model96
    with pytest.raises(RuntimeError, match="weight_from"):
        m.fuse()


# ---------------------------------------------------------------------------------------------------- the planner (tensor-free)
def _plan(N=1, size=512, na=72, **kw):
    defs = parse_model_cfg_text(make_cfg.darknet53_matrix(size, size, na_per_head=na))[1:]
    return defs, plan.plan_eval(defs, mr.matrix_convs(defs), dc._yolos(defs), N, size, size, **kw)


@pytest.mark.parametrize("N", [1, 32])
def test_plan_eval_census_of_the_full_size_cfg(N):
    defs, pl = _plan(N)
    kinds = Counter(op["kind"] for op in pl.ops)
    assert kinds["dconv"] == 36 and kinds["alias"] == 9 and kinds["head"] + kinds["decode"] == 16
    assert kinds["head"] == 16                                      # a shared 1x1 in front of a yolo still takes the fused head-decode launch
    assert "add" not in kinds and "copy" not in kinds
    # every shortcut behind a dconv is folded as its residual: 2 of the 3 dilated convs of each of the 12 branches
    dconvs = [op for op in pl.ops if op["kind"] == "dconv"]
    for op in dconvs:
        i = op["layer"]
        follows = defs[i + 1]["type"] == "shortcut"
        assert (op["res"] is not None) == follows and op["desc"][5:8] == (3, 1, 1)
        if follows:
            assert op["res_layer"] == i - 2 and pl.views[i + 1] == op["out"] and op["res"] == pl.views[i - 2]
        assert op["name"] == "conv_dil<d%dx%d%s>" % (op["dil"] + ("+res" if follows else "",)) and op["src"] == int(defs[i]["weight_from"])
    assert sum(op["res"] is not None for op in dconvs) == 24
    # the aliases: the first 1x1 of every branch of a level but the first -- same input view, same source
    for op in pl.ops:
        if op["kind"] == "alias":
            i, j = op["layer"], op["of"]
            assert defs[i]["weight_from"] == defs[j]["weight_from"] and defs[i - 1]["type"] == "route" and pl.views[i] == pl.views[j]
    assert sorted(int(defs[op["layer"]]["weight_from"]) for op in pl.ops if op["kind"] == "alias") == [75] + [87] * 3 + [99] * 5
    # shared 1x1 layers are ordinary conv ops that name their source
    shared = [op for op in pl.ops if op["kind"] == "conv" and op["src"] is not None]
    assert len(shared) == 48 - 12 - 9 and all(op["desc"][5:8] == (1, 1, 0) for op in shared)
    # and the plain cfg's plan has none of this
    plain = parse_model_cfg_text(make_cfg.darknet53(512, 512))[1:]
    assert all(op.get("src") is None and op["kind"] not in ("dconv", "alias")
               for op in plan.plan_eval(plain, dc._convs(plain), dc._yolos(plain), N, 512, 512).ops)


def test_plan_eval_refuses_what_the_dilated_kernel_does_not_serve():
    defs = parse_model_cfg_text(make_cfg.darknet53_matrix(512, 512))[1:]
    convs = mr.matrix_convs(defs)
    bad = dict(convs)
    bad[114] = dict(convs[114], pad=0)
    with pytest.raises(plan.Refused, match="d-convolutional 114"):
        plan.plan_eval(defs, bad, dc._yolos(defs), 1, 512, 512)
    # C_in 32 in front of a dilated layer: not a multiple of 64
    narrow = dict(convs)
    narrow[113] = dict(convs[113], cout=32)
    with pytest.raises(plan.Refused, match="d-convolutional 114: 32 input channels"):
        plan.plan_eval(defs, narrow, dc._yolos(defs), 1, 512, 512)


def test_plan_train_refuses_matrix_cfgs():
    defs = parse_model_cfg_text(make_cfg.darknet53_matrix(96, 96, na_per_head=8))[1:]
    with pytest.raises(plan.Refused, match="backend = 'torch'"):
        plan.plan_train(defs, mr.matrix_convs(defs), 2, 96, 96)


# ---------------------------------------------------------------------------------------------------- the C ABI, host side
def test_library_exports_the_dilated_entry_points_and_checks_arguments_without_a_gpu():
    L = _lib.lib()
    assert hasattr(L, "ryolo_conv2d_dilated") and hasattr(L, "ryolo_conv2d_dilated_supported")
    vp = C.c_void_p

    def desc(**kw):
        f = dict(N=2, H=9, W=7, Cin=64, Cout=64, ksize=3, stride=1, pad=1, in_cstride=64, out_cstride=64, res_cstride=0,
                 act=ops.ACT_LINEAR, slope=0.1, upsample=1, tile=0)
        f.update(kw)
        return ops.ConvDesc(*[f[n] for n, _ in ops.ConvDesc._fields_])

    def call(d, dh=1, dw=2, x=4096):
        return L.ryolo_conv2d_dilated(C.byref(d), dh, dw, vp(x), vp(4096), vp(4096), vp(4096), None, vp(4096), None)

    assert L.ryolo_conv2d_dilated_supported(C.byref(desc()), 1, 2) == 1
    assert L.ryolo_conv2d_dilated_supported(C.byref(desc(act=ops.ACT_LEAKY, Cout=40, out_cstride=48)), 32, 32) == 1
    for d, dh, dw in ((desc(ksize=1, pad=0), 1, 2), (desc(stride=2), 1, 2), (desc(pad=0), 1, 2), (desc(), 0, 1), (desc(), 1, 33),
                      (desc(Cin=40, in_cstride=40), 1, 2), (desc(act=ops.ACT_MISH), 1, 2), (desc(upsample=2), 1, 2),
                      (desc(Cout=44, out_cstride=48), 1, 2), (desc(out_cstride=56), 1, 2)):
        assert L.ryolo_conv2d_dilated_supported(C.byref(d), dh, dw) == 0
        assert call(d, dh, dw) == -1                      # RYOLO_EINVAL, before any HIP call (this test runs without a GPU)
    assert call(desc(), x=4100) == -1                     # a misaligned pointer
    assert L.ryolo_conv2d_dilated(C.byref(desc()), 1, 2, None, vp(4096), vp(4096), vp(4096), None, vp(4096), None) == -1
    # a residual needs its pixel stride in the descriptor
    assert L.ryolo_conv2d_dilated(C.byref(desc()), 1, 2, vp(4096), vp(4096), vp(4096), vp(4096), vp(4096), vp(4096), None) == -1
