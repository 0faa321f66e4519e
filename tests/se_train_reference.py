"""Test infrastructure for the backward of the squeeze-and-excitation block (csrc/se_bwd.hip, hip_train_ops.SqueezeExcite): the dy
recipe, the block's gradients by fp64 and by fp32 autograd, the terms the data-gradient bar is made of, and a CPU emulation of
SqueezeExcite that rounds where the Function rounds.  Inputs as tests/se_reference.unit_inputs makes them: x NHWC with bf16 values,
w1 [hidden, C] and w2 [C, hidden] fp32."""
import torch

from tests import se_reference as sr


def dy_like(x, seed):
    """the upstream gradient, in the recipe of unit_inputs: randn + U(-2,2)[n,1,1,c], rounded to bf16 (NHWC, x's shape)"""
    n, h, w, c = x.shape
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(n, h, w, c, generator=g) + (torch.rand(n, 1, 1, c, generator=g) * 4 - 2)
    return dy.to(torch.bfloat16)


def direct_weights(c, hidden, seed):
    """weights of unit_inputs' distribution for a hidden width that is not C / 16"""
    g = torch.Generator().manual_seed(seed)
    w1 = (torch.rand(hidden, c, generator=g) * 2 - 1) * (3.0 / c) ** 0.5
    w2 = 2 * (torch.rand(c, hidden, generator=g) * 2 - 1) * (3.0 / hidden) ** 0.5
    return w1.contiguous(), w2.contiguous()


def _autograd(x, dy, w1, w2, dtype):
    xd = x.to(dtype).clone().requires_grad_(True)
    a, b = w1.to(dtype).clone().requires_grad_(True), w2.to(dtype).clone().requires_grad_(True)
    m = xd.mean(dim=(1, 2))
    u = m @ a.t()
    g = torch.sigmoid(torch.relu(u) @ b.t())
    y = xd * g[:, None, None, :]
    y.backward(dy.to(dtype))
    return xd.grad, a.grad, b.grad, g.detach(), u.detach()


def se_bwd_fp64(x, dy, w1, w2):
    """fp64 autograd of the block on the bf16 values -> (dx [N,H,W,C], dW1, dW2, g [N,C], u [N,hidden]), all fp64; computes its own g"""
    return _autograd(x, dy, w1, w2, torch.float64)


def se_bwd_aten_fp32(x, dy, w1, w2):
    """the same by fp32 ATen autograd of SELayer's operator chain (NCHW, adaptive_avg_pool2d, F.linear) -> the same tuple in fp32"""
    import torch.nn.functional as F
    xf = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    a, b = w1.float().clone().requires_grad_(True), w2.float().clone().requires_grad_(True)
    n, c = xf.shape[:2]
    u = F.linear(F.adaptive_avg_pool2d(xf, 1).view(n, c), a)
    g = torch.sigmoid(F.linear(torch.relu(u), b))
    y = xf * g.view(n, c, 1, 1).expand_as(xf)
    y.backward(dy.float().permute(0, 3, 1, 2).contiguous())
    return xf.grad.permute(0, 2, 3, 1).contiguous(), a.grad, b.grad, g.detach(), u.detach()


def se_bwd_terms_fp64(x, dy, w1, w2):
    """the closed form in fp64, term by term: dict(m, u, z, g, s, dt, dz, du, dm_hw [N,C] = dm / (H*W), dyg = dy * g, dx, dw1, dw2)"""
    xd, dd, a, b = x.double(), dy.double(), w1.double(), w2.double()
    hw = x.shape[1] * x.shape[2]
    m = xd.mean(dim=(1, 2))
    u = m @ a.t()
    z = torch.relu(u)
    g = torch.sigmoid(z @ b.t())
    s = (dd * xd).sum(dim=(1, 2))
    dt = s * g * (1 - g)
    dz = dt @ b
    du = torch.where(u > 0, dz, torch.zeros_like(dz))
    dm_hw = (du @ a) / hw
    dyg = dd * g[:, None, None, :]
    return dict(m=m, u=u, z=z, g=g, s=s, dt=dt, dz=dz, du=du, dm_hw=dm_hw, dyg=dyg, dx=dyg + dm_hw[:, None, None, :], dw1=du.t() @ m,
                dw2=dt.t() @ z)


def dx_bar(t, extra=None):
    """the data-gradient bar: 2^-8 (|dy * g64| + |dm64 / (H*W)| [+ |extra|]) + 1e-6 -- one bf16 rounding is 2^-9 of the result, the rest is
    for the fp32 gate and sums"""
    terms = t["dyg"].abs() + t["dm_hw"].abs()[:, None, None, :]
    if extra is not None:
        terms = terms + extra.double().abs()
    return terms * 2.0 ** -8 + 1e-6


def dw_bar(aten, ref):
    """max(1e-6, 8 x fp32 ATen autograd's own relative error on the same operands) -- relative to max|dW64|"""
    scale = float(ref.abs().max())
    return max(1e-6, 8 * float((aten.double() - ref).abs().max()) / max(scale, 1e-300)) * scale


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _gate_fp32(xb, w1, w2):
    """SELayer's own operators on NCHW fp32 -> (m, z, g)"""
    import torch.nn.functional as F
    m = F.adaptive_avg_pool2d(xb, 1).view(xb.shape[0], xb.shape[1])
    z = torch.relu(F.linear(m, w1))
    return m, z, torch.sigmoid(F.linear(z, w2))


class EmulatedSqueezeExcite(torch.autograd.Function):
    """hip_train_ops.SqueezeExcite on the CPU, rounding where it rounds: x and dy to bf16 on entry, fp32 mean / products / gate on the bf16
    values, one bf16 rounding of y and of dx, fp32 weight gradients.  apply(x NCHW fp32, w1, w2) -> NCHW fp32."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        xb = _bf16(x)
        _, _, g = _gate_fp32(xb, w1, w2)
        ctx.save_for_backward(xb, w1, w2)
        return _bf16(xb * g[:, :, None, None])

    @staticmethod
    def backward(ctx, dy):
        xb, w1, w2 = ctx.saved_tensors
        dyb = _bf16(dy)
        hw = xb.shape[2] * xb.shape[3]
        m, z, g = _gate_fp32(xb, w1, w2)
        dt = (dyb * xb).sum(dim=(2, 3)) * g * (1 - g)
        du = torch.where(z > 0, dt @ w2, torch.zeros_like(z))
        dx = _bf16(dyb * g[:, :, None, None] + ((du @ w1) / hw)[:, :, None, None])
        return dx, du.t() @ m, dt.t() @ z


def unit_case(n, h, w, c, hidden=None):
    """(x, dy, w1, w2) of the GPU tier's shape list: unit_inputs(seed = c + h), dy_like(seed = 1000 + c + h); hidden given: weights built
    directly (seed = c + hidden)"""
    x, w1, w2 = sr.unit_inputs(n, h, w, c, seed=c + h)
    if hidden is not None:
        w1, w2 = direct_weights(c, hidden, seed=c + hidden)
    return x, dy_like(x, 1000 + c + h), w1, w2
