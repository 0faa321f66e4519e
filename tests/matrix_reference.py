"""Test infrastructure for the matrix cfgs (shared-weight `weight_from` layers, dilated `d-convolutional` layers): the weight recipe, the
epilogue contract of ryolo_conv2d_dilated restated on the CPU, the planner's input for a cfg (tensor-free), and a layer-by-layer
emulation of a matrix cfg under the engine's bf16 contract.

`forward` is written like tests/se_reference.forward and adds what the reference computes for a block that carries `weight_from = s`
(model/models.py:254-265): x = F.conv2d(x, module_list[s].Conv2d.weight, padding=pad, dilation=dil) -- no bias, BatchNorm or activation,
stride 1.  On a cfg without such blocks it equals the pinned oracle bit for bit (tests/test_matrix_cpu.py)."""
import math

import torch
import torch.nn.functional as F

from oracle import darknet_oracle as do
from rotate_yolov3_amd.model import plan
from tests import dispatch_census as dc
from tests.se_reference import _hash_uniform

# fill_procedural gives a conv weight the values sin(0.37 i + phase) over the flat element index: for one output channel that is a pure
# sinusoid over (c_in, tap), so the conv projects its input onto a single Fourier component -- a rank-2 map.  In the trunk and the FPN path
# BatchNorm shifts and activations add content again after every conv, but a matrix branch is a purely linear chain of seven such convs
# without bias: each one sees only what leaks from its predecessor's sinusoid into its own frequency, the heads end at mean |p| 7e-4 ..
# 2e-2, and they are differences of numbers a thousand times larger: measured on the 96^2 fixture, the fp32 forward then differs from an
# fp64 one by up to 15 x the 1e-5 bars of the CPU golden test (it changes with the number of threads), and a bf16 forward by 15 .. 290 %.
# No common factor on the weights changes that (the chain is linear).  fill_matrix therefore gives every shared SOURCE layer that is not
# a head conv -- the six 1x1 / 3x3 FPN convs of each level -- a full-rank filter instead: an integer hash of (element, layer) in
# [-1, 1) at SHARED_AMP x fill_procedural's amplitude sqrt(3 / fan_in), which keeps a white input's scale.  The head convs keep their
# procedural weights.  With SHARED_AMP 1.0 the matrix heads of the fixture have mean |p| 0.22 .. 1.85 (max 4.1), fp32 against fp64 stays
# within 0.4 x the 1e-5 bars, and what is left of the bf16 sensitivity (7 .. 11 % on the 3^2 and 6^2 levels, 1.2 % on 12^2) is the
# trunk's: its feature maps at layers 61 / 74 differ by 17 % / 8 % between bf16 and fp32, which the FPN heads' single-frequency filters do
# not see and a full-rank filter does.  tests/golden/gen_matrix_golden.py asserts mean |p| >= 0.1 for every matrix head: if it fails,
# change SHARED_AMP.
SHARED_AMP = 1.0


def shared_sources(defs):
    """source layers of the sharing layers of `defs` (cfg dicts without the net block)"""
    return sorted(set(int(d["weight_from"]) for d in defs if "weight_from" in d))


def fill_matrix(model, amp=SHARED_AMP):
    """after fill_procedural: full-rank weights of amplitude amp * sqrt(3 / fan_in) for the shared source convs (head convs excepted)"""
    defs = model.module_defs
    with torch.no_grad():
        for s in shared_sources(defs):
            if defs[s + 1]["type"] == "yolo":
                continue
            w = model.module_list[s].Conv2d.weight
            w.copy_((amp * math.sqrt(3.0 / w[0].numel()) * _hash_uniform(w.numel(), s)).view_as(w).to(w.dtype))
    return model


def matrix_convs(defs):
    """plan_eval's `convs` for a cfg, from its text alone: dispatch_census._convs plus plan.shared_attrs for the sharing layers"""
    convs = dc._convs([d if d["type"] == "convolutional" else dict(type="-") for d in defs])
    for i, d in enumerate(defs):
        if "weight_from" in d:
            convs[i] = plan.shared_attrs(d)
    return convs


def shared_geometry(d):
    """(padding, dilation) of F.conv2d for a block with weight_from (models.py:259-264)"""
    k = int(d["size"])
    if d["type"] == "d-convolutional":
        dil = tuple(int(t) for t in d["dilation"].strip().strip("()").split(","))
        return (dil if int(d.get("pad", 0)) else 0), dil
    return ((k - 1) // 2 if int(d.get("pad", 0)) else 0), 1


# ---------------------------------------------------------------------------------------------------- the kernel's contract
def dilated_reference(x, w, dil, scale=None, shift=None, leaky=None, residual=None):
    """The epilogue contract of include/ryolo.h for ryolo_conv2d_dilated, on the CPU in fp32:
        x [N,H,W,C] bf16, w [Cout,Cin,3,3] fp32 (rounded to bf16 here, as packing does), dil (dh, dw)
        acc = F.conv2d(x, w, padding=dil, dilation=dil) in fp32;  y = bf16(act(acc * scale + shift));  then bf16(y + residual).
    Returns (y as bf16 NHWC, magnitude fp32 NHWC = |value before the add| (+ |residual|): what gets rounded, the scale of the tolerance's
    relative part as in tests/test_conv_gpu.py)."""
    xf = x.float().permute(0, 3, 1, 2).contiguous()
    wf = w.to(torch.bfloat16).float()
    acc = F.conv2d(xf, wf, None, stride=1, padding=tuple(dil), dilation=tuple(dil))
    cout = w.shape[0]
    sc = torch.ones(cout) if scale is None else scale.float()
    sh = torch.zeros(cout) if shift is None else shift.float()
    y = acc * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    if leaky is not None:
        y = torch.where(y > 0, y, y * leaky)
    mag = y.abs()
    y = y.to(torch.bfloat16)
    y = y.permute(0, 2, 3, 1).contiguous()
    mag = mag.permute(0, 2, 3, 1).contiguous()
    if residual is not None:
        y = (y.float() + residual.float()).to(torch.bfloat16)
        mag = mag + residual.float().abs()
    return y, mag


def conv_inputs(n, h, w, cin, cout, seed):
    """inputs scaled as in tests/test_conv_gpu.py: x ~ N(0,1) as NHWC bf16, w ~ N(0,1) / sqrt(9 cin): outputs are O(1)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    return x, wt


# ---------------------------------------------------------------------------------------------------- the model
def forward(cfg_text, sd, x, hyp=None, arc="default", bf16=False, acc64=False, return_layers=False):
    """Eval-mode forward of the cfg graph: tests/se_reference.forward's walk (without se) plus the weight_from layers.  bf16=True: the
    contract of include/ryolo.h -- bf16 tensors and weights, fp32 accumulation, the folded BatchNorm in fp32, one rounding after the
    activation and one after a shortcut.  acc64=True: the same with every conv accumulated in fp64 (the measure of how sensitive a head of
    this model is to the summation order, computed on the CPU alone)."""
    blocks = do.parse_cfg(cfg_text)
    defs = blocks[1:]
    cf = float((hyp or {}).get("context_factor", 1.0))
    img_size = x.shape[-2:]
    r = do._r
    x = r(x.float(), bf16)

    def conv(x, w, **kw):
        if acc64:
            return F.conv2d(x.double(), w.double(), None, **kw).float()
        return F.conv2d(x, w, None, **kw)

    outs, ios, ps = [], [], []
    for i, d in enumerate(defs):
        t = d["type"]
        pre = "module_list.%d." % i
        if "weight_from" in d:
            pad, dil = shared_geometry(d)
            w = r(sd["module_list.%d.Conv2d.weight" % int(d["weight_from"])].float(), bf16)
            x = r(conv(x, w, stride=1, padding=pad, dilation=dil), bf16)
        elif t == "convolutional":
            w = r(sd[pre + "Conv2d.weight"].float(), bf16)
            k = w.shape[-1]
            pad = (k - 1) // 2 if int(d.get("pad", 0)) else 0
            y = conv(x, w, stride=int(d["stride"]), padding=pad)
            if int(d["batch_normalize"]):
                g, b = sd[pre + "BatchNorm2d.weight"].float(), sd[pre + "BatchNorm2d.bias"].float()
                m, v = sd[pre + "BatchNorm2d.running_mean"].float(), sd[pre + "BatchNorm2d.running_var"].float()
                if bf16:
                    scale = g / torch.sqrt(v + 1e-5)
                    shift = b - m * scale
                    y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
                else:
                    y = F.batch_norm(y, m, v, g, b, False, 0.1, 1e-5)
            else:
                y = y + sd[pre + "Conv2d.bias"].float().view(1, -1, 1, 1)
            if d.get("activation") == "leaky":
                y = F.prelu(y, sd[pre + "activation.weight"].float())
            x = r(y, bf16)
        elif t == "upsample":
            x = F.interpolate(x, scale_factor=int(d["stride"]), mode="nearest")
        elif t == "route":
            ls = [int(v) for v in d["layers"].split(",")]
            x = outs[ls[0]] if len(ls) == 1 else torch.cat([outs[l] for l in ls], 1)
        elif t == "shortcut":
            x = r(x + outs[int(d["from"])], bf16)
        elif t == "yolo":
            anchors = do.anchors_of(d["anchors"])[do.mask_of(d["mask"])]
            io, p5 = do.decode(x, anchors, img_size, cf, arc, int(d["classes"]))
            ios.append(io)
            ps.append(p5)
        else:
            raise ValueError("matrix_reference.forward: unknown block type %r" % t)
        outs.append(x)
    res = (torch.cat(ios, 1), ps)
    return res + (outs,) if return_layers else res
