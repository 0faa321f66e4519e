"""CPU tier of training the matrix cfgs with the dilated shared convs on the HIP kernels: the host-side queries of
ryolo_conv2d_dilated_dgrad / ryolo_conv2d_dilated_wgrad (no device call), Darknet.shared_conv_backend, train.py's --backend / --shared-conv,
the exported symbols, and the fairness of the GPU parity bar (tests/test_matrix_train_gpu.py) measured on the emulation alone."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model import hip_train_ops
from rotate_yolov3_amd.model import plan
from rotate_yolov3_amd.model.hip_train_ops import SharedDilatedConv
from rotate_yolov3_amd.utils.parse_config import parse_model_cfg_text
from tests import matrix_reference as mr
from tests import matrix_train_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ryolo_conv2d_dilated_dgrad_supported", "ryolo_conv2d_dilated_dgrad", "ryolo_conv2d_dilated_wgrad_supported",
       "ryolo_conv2d_dilated_wgrad_workspace_bytes", "ryolo_conv2d_dilated_wgrad")


def _T():
    return hip_train_ops


def _desc(**kw):
    f = dict(N=2, H=9, W=7, Cin=64, Cout=64, ksize=3, stride=1, pad=1, in_cstride=64, out_cstride=64, res_cstride=0,
             act=ops.ACT_LINEAR, slope=0.1, upsample=1, tile=0)
    f.update(kw)
    return ops.ConvDesc(*[f[n] for n, _ in ops.ConvDesc._fields_])


def test_new_symbols_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ryolo.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ryolo_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), "libryolo_hip.so does not export %s" % name
    T = _T()
    assert all(name in _lib._sigs for name in NEW) and callable(T.conv_dilated_dgrad) and callable(T.conv_dilated_wgrad)
    assert issubclass(SharedDilatedConv, torch.autograd.Function)


def test_supported_queries_make_no_device_call():
    """served and refused shapes of include/ryolo.h; this test runs on a machine without a GPU"""
    T = _T()
    for cin, cout, n, hw in ((512, 1024, 1, 16), (256, 512, 32, 32), (128, 256, 32, 64)):       # the shapes that matter at 512^2
        for dil in ((1, 2), (2, 1), (1, 4), (4, 1), (1, 8), (8, 1)):
            d = _desc(N=n, H=hw, W=hw, Cin=cin, Cout=cout, in_cstride=cin, out_cstride=cout)
            assert T.conv_dilated_wgrad_supported(d, dil) and T.conv_dilated_dgrad_supported(d, dil)
    assert T.conv_dilated_wgrad_supported(_desc(), (32, 32)) and T.conv_dilated_dgrad_supported(_desc(), (32, 32))
    ragged = _desc(Cout=40, out_cstride=64)                      # a ragged C_out: the weight gradient serves it, the data gradient does not
    assert T.conv_dilated_wgrad_supported(ragged, (1, 2)) and not T.conv_dilated_dgrad_supported(ragged, (1, 2))
    assert T.conv_dilated_wgrad_supported(_desc(Cout=96, out_cstride=96), (1, 2))
    assert not T.conv_dilated_dgrad_supported(_desc(Cout=96, out_cstride=96), (1, 2))         # C_out is the data gradient's K channel count
    for d, dil in ((_desc(Cin=32, in_cstride=32), (1, 2)), (_desc(), (0, 1)), (_desc(), (1, 0)), (_desc(), (33, 1)), (_desc(), (1, 33)),
                   (_desc(ksize=1, pad=0), (1, 2)), (_desc(stride=2), (1, 2)), (_desc(pad=0), (1, 2)), (_desc(upsample=2), (1, 2)),
                   (_desc(Cout=44, out_cstride=48), (1, 2)), (_desc(out_cstride=56), (1, 2)), (_desc(in_cstride=60), (1, 2)),
                   (_desc(N=1 << 12, H=1 << 10, W=1 << 10), (1, 2))):                     # 2^32 pixels: past the 2 GiB tensors
        assert not T.conv_dilated_wgrad_supported(d, dil), (tuple(getattr(d, n) for n, _ in d._fields_), dil)
        assert not T.conv_dilated_dgrad_supported(d, dil)
        assert T.conv_dilated_wgrad_ws_bytes(d, dil) == 0


def test_workspace_query_and_split_depend_on_the_shape_alone():
    T = _T()
    # [S][cpad128(Cout)][9 Cin] fp32; S = floor(512 / (9 * c_out tiles * c_in tiles)) capped at one split per 64-pixel K step
    assert T.conv_dilated_wgrad_ws_bytes(_desc(), (1, 2)) == 2 * 128 * 9 * 64 * 4                               # 126 pixels: 2 steps
    d = _desc(N=3, H=12, W=12, Cin=128, Cout=256, in_cstride=128, out_cstride=256)
    assert T.conv_dilated_wgrad_ws_bytes(d, (4, 1)) == 7 * 256 * 9 * 128 * 4
    assert T.conv_dilated_wgrad_ws_bytes(d, (1, 2)) == T.conv_dilated_wgrad_ws_bytes(d, (4, 1))                 # not on the dilation
    for n in (1, 32):          # the tile list fills 256 CUs at the shapes that matter: at least 256 workgroups
        for cin, cout, hw in ((512, 1024, 16), (256, 512, 32), (128, 256, 64)):
            d = _desc(N=n, H=hw, W=hw, Cin=cin, Cout=cout, in_cstride=cin, out_cstride=cout)
            s = T.conv_dilated_wgrad_ws_bytes(d, (1, 2)) // (cout * 9 * cin * 4)
            assert s >= 1 and 9 * (cout // 128) * (cin // 128) * s >= 256, (n, cin, cout, s)


def test_calls_refuse_bad_arguments_before_any_device_call():
    L = _lib.lib()
    _T()
    vp = C.c_void_p

    def wg(d, dil=(1, 2), x=4096, dz=4096, g=4096, ws=4096, wsb=1 << 30, dz_cs=None):
        return L.ryolo_conv2d_dilated_wgrad(C.byref(d), dil[0], dil[1], vp(x) if x else None, vp(dz) if dz else None,
                                            d.Cout if dz_cs is None else dz_cs, vp(g) if g else None, 0, vp(ws) if ws else None, wsb, None)

    def dg(d, dil=(1, 2), dz=4096, pk=4096, dx=4096):
        return L.ryolo_conv2d_dilated_dgrad(C.byref(d), dil[0], dil[1], vp(dz) if dz else None, d.Cout, vp(pk) if pk else None, vp(4096),
                                            vp(4096), vp(dx) if dx else None, None)

    assert wg(_desc(Cin=32, in_cstride=32)) == -1 and dg(_desc(Cin=32, in_cstride=32)) == -1
    assert dg(_desc(Cout=96, out_cstride=96)) == -1
    for dil in ((0, 1), (33, 1), (1, 0), (1, 33)):
        assert wg(_desc(), dil) == -1 and dg(_desc(), dil) == -1
    assert wg(_desc(), wsb=2 * 128 * 9 * 64 * 4 - 1) == -1                     # a short workspace
    for k in ("x", "dz", "g", "ws"):
        assert wg(_desc(), **{k: 0}) == -1                                      # a null pointer
    for k in ("dz", "pk", "dx"):
        assert dg(_desc(), **{k: 0}) == -1
    assert wg(_desc(), x=4100) == -1 and dg(_desc(), dz=4100) == -1            # a misaligned pointer
    assert wg(_desc(), dz_cs=60) == -1


# ---------------------------------------------------------------------------------------------------- the model attribute
def test_shared_conv_backend_attribute():
    m = R.make_model()
    assert m.shared_conv_backend == "torch"
    with pytest.raises(ValueError, match="shared_conv_backend"):
        m.shared_conv_backend = "triton"
    assert m.shared_conv_backend == "torch"
    x = R.make_input()
    rs = R.fixed_r(m(x))
    want = R.grads(m, m(x), rs)
    m.shared_conv_backend = "hip"                      # a CPU forward ignores it: the same ATen chain, the same bits
    got = R.grads(m, m(x), rs)
    assert all(torch.equal(got[k], want[k]) for k in want)
    plain = R.grads(m, R.chain(m, x), rs)
    assert all(torch.equal(plain[k], want[k]) for k in want)
    assert "shared_conv_packs" not in m.__dict__       # nothing was packed


def test_plan_train_still_refuses_matrix_cfgs():
    defs = parse_model_cfg_text(make_cfg.darknet53_matrix(96, 96, na_per_head=8))[1:]
    with pytest.raises(plan.Refused, match="backend = 'torch'"):
        plan.plan_train(defs, mr.matrix_convs(defs), 2, 96, 96)
    defs = parse_model_cfg_text(R.MINI_CFG)[1:]
    with pytest.raises(plan.Refused):
        plan.plan_train(defs, mr.matrix_convs(defs), 2, 64, 64)


# ---------------------------------------------------------------------------------------------------- train.py
def test_train_py_arguments():
    sys.path.insert(0, ROOT)
    import train
    _, _, opt = train.parse_args([])
    assert opt.backend == "hip" and opt.shared_conv == "torch"
    _, _, opt = train.parse_args(["--backend", "torch", "--shared-conv", "hip"])
    assert opt.backend == "torch" and opt.shared_conv == "hip"
    for bad in (["--shared-conv", "hip", "--backend", "hip"], ["--shared-conv", "hip"], ["--backend", "aten"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2


def test_train_py_backend_torch_trains_a_matrix_cfg(tmp_path):
    """--backend torch reaches Darknet._torch_forward: a cfg with weight_from / d-convolutional layers, which the TrainEngine refuses,
    trains from the command line; --shared-conv hip --backend hip is an argument error"""
    cfg = tmp_path / "m.cfg"
    cfg.write_text(R.MINI_CFG)
    hyp = tmp_path / "hyp.py"
    hyp.write_text("giou: 0.1\ncls: 27.76\ncls_pw: 1.446\nobj: 20.35\nobj_pw: 3.941\niou_t: 0.3\nang_t: 3.1415926/12\n"
                   "reg: 1.0\nfl_gamma: 0.5\ncontext_factor: 1.0\nlr0: 0.0001\nmultiplier:10\nwarm_epoch:1\nmomentum: 0.97\n"
                   "weight_decay: 0.0004569\nepochs: 1\nbatch_size: 2\nsave_interval: 300\ntest_interval: 5\n")
    base = [sys.executable, os.path.join(ROOT, "train.py"), "--cfg", str(cfg), "--hyp", str(hyp), "--img-size", "64", "--synthetic", "2",
            "--device", "cpu", "--wdir", str(tmp_path / "w")]
    r = subprocess.run(base + ["--backend", "torch"], cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "backend='torch'" in r.stdout and "shared_conv='torch'" in r.stdout
    assert os.path.isfile(str(tmp_path / "w" / "last.pt"))
    r = subprocess.run(base + ["--shared-conv", "hip", "--backend", "hip"], cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 2 and "--shared-conv hip needs --backend torch" in r.stderr, r.stderr[-800:]


# ---------------------------------------------------------------------------------------------------- is the GPU parity bar fair?
def test_parity_bar_is_at_least_twice_the_emulations_own_accumulation_error():
    """tests/test_matrix_train_gpu.py holds the HIP chain to max|err| <= 2e-3 max|g| + 1e-3 against the fp32-accumulating emulation.  The
    kernels sum in another order than ATen does, so the bar must leave room for that: the emulation with fp64 accumulation against the
    one with fp32 accumulation stays inside half the bar (measured: 6.4e-3 of a half bar of 0.22 for the stem, 4.1e-3 of 0.18 for A)"""
    m = R.make_model()
    x = R.make_input()
    rs = R.fixed_r(m(x))
    g32 = R.grads(m, R.chain(m, x, R.emulated(torch.float32)), rs)
    g64 = R.grads(m, R.chain(m, x, R.emulated(torch.float64)), rs)
    for k in (R.STEM, R.A):
        err = float((g32[k] - g64[k]).abs().max())
        print("layer %d: fp64 vs fp32 accumulation %.4g, half bar %.4g" % (k, err, 0.5 * R.dw_bar(g64[k])))
        assert err <= 0.5 * R.dw_bar(g64[k])
        assert R.cosine(g32[k], g64[k]) >= 0.9999
