"""Test infrastructure for training a matrix cfg through the ATen chain with the dilated shared convs on the HIP kernels
(Darknet.shared_conv_backend = 'hip'): a mini cfg, a restatement of Darknet._torch_forward with a pluggable dilated conv, the CPU emulation
of hip_train_ops.SharedDilatedConv (bf16 roundings where the Function has them, fp32 or fp64 accumulation), and the scalar the tests
differentiate."""
import torch
import torch.nn.functional as F

from rotate_yolov3_amd.model.models import Darknet, shared_conv_geometry

# layer 0: stride-2 stem to 64 channels; 1: the 3x3 64 -> 64 source layer A; 2, 3: its head and yolo; 4: route back to the stem's output;
# 5, 6: two d-convolutional layers sharing A's weight, dilations (1,2) and (2,1); 7: shortcut; 8, 9: a head sharing the first head's weight
MINI_CFG = """
[net]
width=64
height=64
channels=3

[convolutional]
batch_normalize=1
filters=64
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=84
activation=linear

[yolo]
mask = 0-11
anchors = 20,8, 60,20
classes=1
num=2

[route]
layers = -4

[d-convolutional]
dilation=(1,2)
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky
weight_from = 1

[d-convolutional]
dilation=(2,1)
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky
weight_from = 1

[shortcut]
from=-3
activation=linear

[convolutional]
size=1
stride=1
pad=1
filters=84
activation=linear
weight_from = 2

[yolo]
mask = 12-23
anchors = 20,8, 60,20
classes=1
num=2
"""
STEM, A, SHARERS = 0, 1, (5, 6)


def make_model(seed=0):
    torch.manual_seed(seed)
    return Darknet(MINI_CFG, {"context_factor": 1.0}).train()


def make_input(seed=1, n=2):
    return torch.rand(n, 3, 64, 64, generator=torch.Generator().manual_seed(seed))


def fixed_r(ps, seed=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g) for p in ps]


def scalar(ps, rs):
    """sum_k <p_k, r_k> with fixed random r_k: linear in the heads, so no loss code is under test"""
    return sum((p * r.to(p.device)).sum() for p, r in zip(ps, rs))


def chain(model, x, dconv=None):
    """Darknet._torch_forward in training mode, restated: `convolutional` blocks run their module, a block with weight_from runs
    F.conv2d with the source layer's weight and nothing else -- or dconv(x, weight, dil) for the d-convolutional ones when given"""
    outs, heads = [], []
    for i, (d, m) in enumerate(zip(model.module_defs, model.module_list)):
        t = d["type"]
        if "weight_from" in d:
            _, pad, dil = shared_conv_geometry(d)
            w = model.module_list[int(d["weight_from"])].Conv2d.weight
            if t == "d-convolutional" and dconv is not None:
                x = dconv(x, w, tuple(dil))
            else:
                x = F.conv2d(x, w, padding=pad, dilation=dil)
        elif t == "convolutional":
            x = m(x)
        elif t == "route":
            x = outs[int(d["layers"])]
        elif t == "shortcut":
            x = x + outs[int(d["from"])]
        elif t == "yolo":
            x = m(x, (64, 64))
            heads.append(x)
        else:
            raise ValueError(t)
        outs.append(x)
    return heads


def _bf(t):
    return t.to(torch.bfloat16).float()


class EmulatedSharedDilatedConv(torch.autograd.Function):
    """hip_train_ops.SharedDilatedConv on the CPU: x, W and dy rounded to bf16 where the Function converts them, the products accumulated
    in `acc` (torch.float32 or torch.float64), y and dx rounded to bf16 where the kernels store them, dW left in fp32"""

    @staticmethod
    def forward(ctx, x, w, dil, acc):
        xb, wb = _bf(x), _bf(w)
        ctx.save_for_backward(xb, wb)
        ctx.dil, ctx.acc = dil, acc
        return _bf(F.conv2d(xb.to(acc), wb.to(acc), padding=dil, dilation=dil).float())

    @staticmethod
    def backward(ctx, dy):
        xb, wb = ctx.saved_tensors
        dil, acc = ctx.dil, ctx.acc
        dyb = _bf(dy).to(acc)
        dx = torch.nn.grad.conv2d_input(xb.shape, wb.to(acc), dyb, padding=dil, dilation=dil)
        dw = torch.nn.grad.conv2d_weight(xb.to(acc), wb.shape, dyb, padding=dil, dilation=dil)
        return _bf(dx.float()), dw.float(), None, None


def emulated(acc=torch.float32):
    return lambda x, w, dil: EmulatedSharedDilatedConv.apply(x, w, dil, acc)


def grads(model, heads, rs):
    """{layer: Conv2d.weight.grad} of the stem and A after backward of the scalar"""
    model.zero_grad(set_to_none=True)
    scalar(heads, rs).backward()
    return {k: model.module_list[k].Conv2d.weight.grad.detach().clone() for k in (STEM, A)}


def cosine(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm()))


def dw_bar(want):
    """the project's per-block dW bar: max|err| <= 2e-3 max|g| + 1e-3, cosine >= 0.9999"""
    return 2e-3 * float(want.abs().max()) + 1e-3
