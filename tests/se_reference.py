"""Test infrastructure for the squeeze-and-excitation layers: weight / input recipes, an fp64 statement of the block, and a
layer-by-layer emulation of an se cfg under the engine's bf16 contract.

`forward` is written like oracle.darknet_oracle.forward (which passes over block types it does not know and so cannot serve the
se cfgs) and adds the `se` block; on a cfg without se blocks it must equal that function bit for bit (tests/test_se_cpu.py), which
ties this helper to the pinned oracle."""
import math

import torch
import torch.nn.functional as F

from oracle import darknet_oracle as do

# fill_se amplitude, in units of sqrt(3 / fan_in) for fc.0 and 2 * sqrt(3 / fan_in) for fc.2.  tests/golden/gen_se_golden.py asserts that
# with it every se layer of darknet53_se(64, 64) on the golden input has gates below 0.35 and above 0.65 (fill_procedural alone
# would give the fc tensors amplitude 0.05: every gate ~0.5, and a kernel that ignored the pool would pass).  With 1.0 layer 37 stayed in
# [0.368, 0.620]; 2.0 passes at every layer.
SE_AMP = 2.0


def _hash_uniform(n, salt):
    """n values in [-1, 1): an integer hash of (index, salt), exact in int64 -- the same on every machine"""
    i = torch.arange(n, dtype=torch.int64)
    h = (i * 2654435761 + salt * 40503 + 12345) % (1 << 32)
    h = h ^ (h >> 15)
    h = (h * 1103515245 + 12345) % (1 << 32)
    h = h ^ (h >> 13)
    h = (h * 1664525 + 1013904223) % (1 << 32)
    h = h ^ (h >> 16)
    return h.to(torch.float64) / float(1 << 31) - 1.0


def fill_se(model, amp=SE_AMP):
    """overwrite the fc weights of every SELayer (after fill_procedural): a deterministic function of (state_dict position, element)"""
    sd = model.state_dict()
    with torch.no_grad():
        for li, (name, t) in enumerate(sd.items()):
            if name.endswith(".fc.0.weight") or name.endswith(".fc.2.weight"):
                fan_in = t.shape[1]
                a = amp * math.sqrt(3.0 / fan_in) * (2.0 if name.endswith(".fc.2.weight") else 1.0)
                t.copy_((a * _hash_uniform(t.numel(), li)).view_as(t).to(t.dtype))
    return model


def unit_inputs(n, h, w, c, seed=0):
    """the unit-level recipe: x = randn + U(-2,2)[n,c] as NHWC bf16, W1 = U(-1,1) sqrt(3/C), W2 = 2 U(-1,1) sqrt(3/hidden), fp32"""
    g = torch.Generator().manual_seed(seed)
    hidden = c // 16
    x = torch.randn(n, h, w, c, generator=g) + (torch.rand(n, 1, 1, c, generator=g) * 4 - 2)
    w1 = (torch.rand(hidden, c, generator=g) * 2 - 1) * math.sqrt(3.0 / c)
    w2 = 2 * (torch.rand(c, hidden, generator=g) * 2 - 1) * math.sqrt(3.0 / hidden)
    return x.to(torch.bfloat16), w1.contiguous(), w2.contiguous()


def se_fp64(x, w1, w2):
    """x NHWC (bf16 values), fp32 weights -> (fp64 x * gate [N,H,W,C], fp64 gate [N,C])"""
    xd = x.double()
    m = xd.mean(dim=(1, 2))
    g = torch.sigmoid(torch.relu(m @ w1.double().t()) @ w2.double().t())
    return xd * g[:, None, None, :], g


def se_aten_fp32(x, w1, w2):
    """the reference's own operator chain in fp32 (SELayer.forward) on the same values -> (y fp32 NHWC, gate fp32)"""
    xf = x.float().permute(0, 3, 1, 2).contiguous()
    b, c = xf.shape[:2]
    m = F.adaptive_avg_pool2d(xf, 1).view(b, c)
    g = torch.sigmoid(F.linear(torch.relu(F.linear(m, w1)), w2))
    return (xf * g.view(b, c, 1, 1)).permute(0, 2, 3, 1), g


def bf16_ulp_diff(a, b):
    """distance in bf16 steps between two bf16 tensors (ordered-integer view of the bit patterns)"""
    def key(t):
        v = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(v >= 0x8000, 0x8000 - v, v)
    return (key(a) - key(b)).abs()


def forward(cfg_text, sd, x, hyp=None, arc="default", bf16=False, return_gates=False, return_layers=False):
    """Eval-mode forward of the cfg graph, darknet_oracle.forward plus the `se` block.  bf16=True: the contract of include/ryolo.h --
    bf16 tensors, fp32 pool / products / gate on the bf16 values, one rounding of x * gate."""
    blocks = do.parse_cfg(cfg_text)
    defs = blocks[1:]
    cf = float((hyp or {}).get("context_factor", 1.0))
    img_size = x.shape[-2:]
    r = do._r
    x = r(x.float(), bf16)
    outs, ios, ps, gates = [], [], [], []
    for i, d in enumerate(defs):
        t = d["type"]
        pre = "module_list.%d." % i
        if t == "convolutional":
            w = r(sd[pre + "Conv2d.weight"].float(), bf16)
            k = w.shape[-1]
            pad = (k - 1) // 2 if int(d.get("pad", 0)) else 0
            y = F.conv2d(x, w, None, stride=int(d["stride"]), padding=pad)
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
        elif t == "se":
            bsz, c = x.shape[:2]
            m = F.adaptive_avg_pool2d(x, 1).view(bsz, c)
            g = torch.sigmoid(F.linear(torch.relu(F.linear(m, sd[pre + "fc.0.weight"].float())), sd[pre + "fc.2.weight"].float()))
            gates.append(g)
            x = r(x * g.view(bsz, c, 1, 1), bf16)
        elif t == "maxpool":
            k, s = int(d["size"]), int(d["stride"])
            if k == 2 and s == 1:
                x = F.max_pool2d(F.pad(x, (0, 1, 0, 1)), k, s, 0)
            else:
                x = F.max_pool2d(x, k, s, (k - 1) // 2)
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
            raise ValueError("se_reference.forward: unknown block type %r" % t)
        outs.append(x)
    res = (torch.cat(ios, 1), ps)
    if return_layers:
        res = res + (outs,)
    return res + (gates,) if return_gates else res
