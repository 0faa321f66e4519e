"""Backward references for the dilated shared convs (ryolo_conv2d_dilated_dgrad / ryolo_conv2d_dilated_wgrad, SharedDilatedConv): fp32 ATen
autograd on the CPU on the SAME bf16-rounded operands the kernels read, computed once per case and shared by the tests that need them
(the results are cached: do not modify them in place).

    y  = F.conv2d(x, W, padding=dil, dilation=dil)                          3x3, stride 1
    dx = autograd's gradient of <y, dy> with respect to x,  dW = ... with respect to W
    terms = the same dx with |dy| and |W|: sum over the products' magnitudes, the scale of the data gradient's tolerance"""
import functools

import torch
import torch.nn.functional as F

from tests import matrix_reference as mr

WGRAD_REL, WGRAD_ABS = 2e-3, 1e-3        # the bar of tests/test_train_ops_gpu.py::test_wgrad_vs_autograd: max|err| <= 2e-3 max|dW| + 1e-3
DGRAD_REL, DGRAD_ABS = 2.0 ** -7, 2e-3   # the dilated forward's bar (tests/test_conv_dil_gpu.py) over the summed magnitudes of the terms


@functools.lru_cache(maxsize=None)
def bwd_inputs(n, h, w, cin, cout, seed):
    """x [N,H,W,Cin] bf16 and W [Cout,Cin,3,3] fp32 of matrix_reference.conv_inputs, plus dy [N,H,W,Cout] ~ N(0,1) bf16"""
    x, wt = mr.conv_inputs(n, h, w, cin, cout, seed)
    dy = torch.randn(n, h, w, cout, generator=torch.Generator().manual_seed(seed + 5000)).to(torch.bfloat16)
    return x, wt, dy


def _nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous()


def conv_backward(x, wt, dy, dil):
    """(y, dx, dW) in fp32 from NHWC bf16 x / dy and fp32 OIHW W (rounded to bf16 here, as packing does); y, dx as NHWC"""
    xf = _nchw(x).requires_grad_(True)
    wf = wt.to(torch.bfloat16).float().requires_grad_(True)
    y = F.conv2d(xf, wf, None, stride=1, padding=tuple(dil), dilation=tuple(dil))
    dx, dw = torch.autograd.grad(y, (xf, wf), _nchw(dy))
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous(), dw


@functools.lru_cache(maxsize=None)
def reference(n, h, w, cin, cout, dil, seed):
    """dict(x, w, dy, y, dx, dw) for one case"""
    x, wt, dy = bwd_inputs(n, h, w, cin, cout, seed)
    y, dx, dw = conv_backward(x, wt, dy, dil)
    return dict(x=x, w=wt, dy=dy, y=y, dx=dx, dw=dw)


@functools.lru_cache(maxsize=None)
def dgrad_terms(n, h, w, cin, cout, dil, seed):
    """sum of |dy| |W| over the terms of every dx element (NHWC fp32)"""
    x, wt, dy = bwd_inputs(n, h, w, cin, cout, seed)
    return conv_backward(x, wt.to(torch.bfloat16).float().abs(), dy.abs(), dil)[1]


def wgrad_bar(want):
    return WGRAD_REL * want.abs().max().item() + WGRAD_ABS


def check_wgrad(got, want, what=""):
    err = (got.detach().float().cpu() - want).abs().max().item()
    bar = wgrad_bar(want)
    print("%s dW: max err %.4g, bar %.4g, max |dW| %.4g" % (what, err, bar, want.abs().max().item()))
    assert err <= bar, "%s dW: max err %.4g above %.4g" % (what, err, bar)


def check_dgrad(got, want, terms, what=""):
    err = (got.detach().float().cpu() - want).abs()
    tol = DGRAD_REL * terms + DGRAD_ABS
    print("%s dx: max err %.4g, mean |dx| %.3g" % (what, err.max().item(), want.abs().mean().item()))
    assert bool((err <= tol).all()), "%s dx: max err %.4g (tol %.4g there)" % (what, err.max().item(), tol.flatten()[err.argmax()].item())
