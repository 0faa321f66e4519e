"""CPU tier of the squeeze-and-excitation backward: the host-side checks of ryolo_se_bwd_workspace_bytes / ryolo_se_bwd_nhwc (no device
call), Darknet.se_backend, train.py's --se, and the CPU emulation of SqueezeExcite (tests/se_train_reference.py) against fp32 autograd
of SELayer within the rounding it adds."""
import ctypes as C
import os
import pickle
import re
import sys

import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_train_ops as T
from rotate_yolov3_amd.model.models import Darknet, SELayer
from tests import se_reference as sr
from tests import se_train_reference as R
from tests.procedural import fill_procedural

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ryolo_se_bwd_workspace_bytes", "ryolo_se_bwd_nhwc")
EINVAL = -1


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ryolo.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ryolo_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib._sigs, name
        assert hasattr(raw, name), "libryolo_hip.so does not export %s" % name
    assert _lib.lib().ryolo_abi_version() == 4
    assert callable(T.se_bwd_ws_bytes) and callable(T.se_bwd_nhwc) and issubclass(T.SqueezeExcite, torch.autograd.Function)


def test_workspace_query_makes_no_device_call():
    ws = T.se_bwd_ws_bytes
    sizes = [ws(n, 76, 76, 256, 16) for n in (1, 2, 3, 8, 32)]
    assert all(a > 0 for a in sizes) and all(a < b for a, b in zip(sizes[:-1], sizes[1:]))          # grows with N
    # at least the row pairs of the 46 chunks of a 76 x 76 x 256 image (csrc/se.hip) and the g / dm rows
    assert ws(32, 76, 76, 256, 16) >= 32 * (46 * 2 + 2) * 256 * 4
    assert ws(1, 1, 1, 16, 1) > 0 and ws(1, 3, 3, 2048, 128) > 0 and ws(65535, 1, 1, 16, 1) > 0
    assert ws(1, 8, 8, 256, 17) > ws(1, 8, 8, 256, 16)                                              # and with the hidden width
    for bad in ((1, 8, 8, 12, 1), (1, 8, 8, 4096, 16), (0, 8, 8, 64, 4), (1, 8, 8, 8, 1), (1, 8, 8, 64, 0), (1, 8, 8, 64, 129),
                (65536, 8, 8, 64, 4), (1, 0, 8, 64, 4), (1, 8, -1, 64, 4), (1, 1 << 16, 1 << 16, 64, 4)):
        assert ws(*bad) == 0, bad


def test_every_einval_is_returned_before_any_launch():
    """the pointers are never dereferenced and nothing is enqueued: this runs on a machine without a GPU"""
    lib = _lib.lib()
    vp = C.c_void_p
    MB = 1 << 20
    need = T.se_bwd_ws_bytes(1, 8, 8, 256, 16)

    def call(x=1 * MB, xcs=256, dy=2 * MB, dycs=256, w1=3 * MB, w2=4 * MB, hidden=16, dx=5 * MB, dxcs=256, dxacc=0, dw1=6 * MB, dw2=7 * MB,
             accw=0, N=1, H=8, W=8, Cc=256, gate=None, wsp=8 * MB, nbytes=1 << 30):
        p = [vp(a) if a else None for a in (x, dy, w1, w2, dx, dw1, dw2, gate, wsp)]
        return lib.ryolo_se_bwd_nhwc(p[0], xcs, p[1], dycs, p[2], p[3], hidden, p[4], dxcs, dxacc, p[5], p[6], accw, N, H, W, Cc, p[7], p[8],
                                     C.c_size_t(nbytes), None)
    # a required null pointer
    for k in ("x", "dy", "w1", "w2", "wsp"):
        assert call(**{k: 0}) == EINVAL, k
    # one weight gradient alone; nothing asked for
    assert call(dw1=0) == EINVAL and call(dw2=0) == EINVAL
    assert call(dx=0, dw1=0, dw2=0) == EINVAL
    # a size outside the range
    assert call(Cc=12, xcs=16, dycs=16, dxcs=16) == EINVAL and call(Cc=8, xcs=8, dycs=8, dxcs=8) == EINVAL
    assert call(Cc=4096, xcs=4096, dycs=4096, dxcs=4096) == EINVAL
    assert call(hidden=0) == EINVAL and call(hidden=129) == EINVAL
    assert call(N=0) == EINVAL and call(N=65536) == EINVAL and call(H=0) == EINVAL and call(W=-3) == EINVAL
    # strides: >= C, multiples of 8
    for k in ("xcs", "dycs", "dxcs"):
        assert call(**{k: 248}) == EINVAL and call(**{k: 260}) == EINVAL, k
    # alignment: bf16 bases 16 bytes, fp32 pointers 4 bytes, workspace 16 bytes
    for k in ("x", "dy", "dx", "wsp"):
        assert call(**{k: 9 * MB + 8}) == EINVAL, k
    for k in ("w1", "w2", "dw1", "dw2", "gate"):
        assert call(**{k: 9 * MB + 2}) == EINVAL, k
    # a short workspace
    assert need > 0 and call(nbytes=need - 1) == EINVAL
    # dx overlapping x or dy, by the rule of ryolo_se_nhwc
    assert call(dx=1 * MB) == EINVAL and call(dx=2 * MB) == EINVAL
    assert call(dx=1 * MB + 64) == EINVAL and call(dx=2 * MB + 64) == EINVAL
    assert call(xcs=512, dxcs=512, dx=1 * MB + 256) == EINVAL                   # slices of one buffer whose channel intervals meet
    assert call(dycs=512, dxcs=512, dx=2 * MB + 2 * 128) == EINVAL
    assert call(dycs=512, dxcs=384, dx=2 * MB + 2 * 256) == EINVAL              # meeting ranges with different strides
    # (the accepted forms -- disjoint slices of one buffer, optional outputs left out -- launch: tests/test_se_bwd_gpu.py)


def _se_model():
    return sr.fill_se(fill_procedural(Darknet(make_cfg.darknet53_se(64, 64), {"context_factor": 1.0})))


def _grads(m, x, rs):
    m.zero_grad(set_to_none=True)
    ps = m(x)
    sum((p * r).sum() for p, r in zip(ps, rs)).backward()
    return ps, {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}


def test_se_backend_attribute():
    m = _se_model()
    assert m.se_backend == "torch"
    for bad in ("triton", "HIP", None, 1):
        with pytest.raises(ValueError, match="se_backend"):
            m.se_backend = bad
    assert m.se_backend == "torch"
    m.backend = "torch"
    m.train()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    g = torch.Generator().manual_seed(4)
    rs = [torch.randn(p.shape, generator=g) for p in m(x)]
    p0, want = _grads(m, x, rs)
    m.se_backend = "hip"                               # a CPU forward ignores it: the same ATen chain, the same bits
    assert m.se_backend == "hip"
    p1, got = _grads(m, x, rs)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert "module_list.13.fc.0.weight" in want and float(want["module_list.13.fc.0.weight"].abs().max()) > 0
    # a model pickled before the attribute existed reads as the default
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.se_backend == "hip"
    del m2.__dict__["_se_backend"]
    assert m2.se_backend == "torch"


def test_squeeze_excite_raises_on_cpu_tensors():
    x, w1, w2 = sr.unit_inputs(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        T.SqueezeExcite.apply(x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True), w1, w2)


def test_train_py_arguments():
    sys.path.insert(0, ROOT)
    import train
    _, _, opt = train.parse_args([])
    assert opt.backend == "hip" and opt.se == "torch"
    _, _, opt = train.parse_args(["--se", "hip", "--backend", "torch"])
    assert opt.backend == "torch" and opt.se == "hip"
    _, _, opt = train.parse_args(["--backend", "torch"])
    assert opt.se == "torch"
    for bad in (["--se", "hip"], ["--se", "hip", "--backend", "hip"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        train.parse_args(["--se", "aten", "--backend", "torch"])


def test_train_py_se_hip_error_message(capsys):
    sys.path.insert(0, ROOT)
    import train
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--se", "hip", "--backend", "hip"])
    assert e.value.code == 2
    assert "--se hip needs --backend torch" in capsys.readouterr().err


@pytest.mark.parametrize("shape", [(2, 8, 8, 256), (3, 5, 7, 64), (2, 6, 6, 40)], ids=lambda s: "x".join(map(str, s)))
def test_emulation_against_fp32_autograd_of_selayer(shape):
    """EmulatedSqueezeExcite rounds x and dy to bf16 on entry and y and dx once on exit.  On inputs that already are bf16 values the
    entry roundings do nothing, so against fp32 autograd of SELayer on the same values: y and dx differ by their one bf16 rounding
    (relative 2^-9, plus fp32 noise: 2^-8 of the terms' magnitudes + 1e-6), the weight gradients by fp32 summation order alone
    (1e-5 of their largest element)."""
    n, h, w, c = shape
    x, dy, w1, w2 = R.unit_case(n, h, w, c)
    se = SELayer(c)
    with torch.no_grad():
        se.fc[0].weight.copy_(w1)
        se.fc[2].weight.copy_(w2)
    xa = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ya = se(xa)
    ya.backward(dy.float().permute(0, 3, 1, 2).contiguous())
    xe = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    a, b = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    ye = R.EmulatedSqueezeExcite.apply(xe, a, b)
    ye.backward(dy.float().permute(0, 3, 1, 2).contiguous())
    assert torch.equal(ye.detach(), ya.detach().to(torch.bfloat16).float())          # the forward: fp32 ATen's y, rounded once
    t = R.se_bwd_terms_fp64(x, dy, w1, w2)
    bar = R.dx_bar(t).permute(0, 3, 1, 2)
    err = (xe.grad.double() - xa.grad.double()).abs()
    assert bool((err <= bar).all()), float((err / bar).max())
    assert torch.equal(xe.grad, xe.grad.to(torch.bfloat16).float())                  # dx is a bf16 value
    for got, want in ((a.grad, se.fc[0].weight.grad), (b.grad, se.fc[2].weight.grad)):
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
