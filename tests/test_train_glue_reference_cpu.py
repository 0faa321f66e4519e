"""The fp64 references of tests/train_glue_reference.py checked against independent formulations, without a GPU: the backward reference
against fp64 autograd through F.batch_norm(training=True) and the activation, the forward reference's two roundings on planted ties, the
finalize reference against torch.nn.BatchNorm2d in fp64, and the bf16 rounding helper against torch's fp32 -> bf16 conversion."""
import pytest
import torch
import torch.nn.functional as F

from tests.train_glue_reference import (BF, F64, bn_act_bwd_ref, bn_act_fwd_ref, bn_finalize_ref, pgrad_to_nhwc_ref, rn_bf16,
                                        upsample2x_bwd_ref)

EPS = 1e-5


def _close(got, want, rel=1e-10):
    want = want.to(F64)
    return bool(((got - want).abs() <= rel * want.abs() + rel * want.abs().max()).all())


def test_rn_bf16_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(20000, generator=g) * torch.exp2(torch.randint(-20, 20, (20000,), generator=g).float())
    assert torch.equal(rn_bf16(x.double()), x.to(BF).double())       # fp32 -> bf16 in torch is one correctly rounded step
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 257.0, 259.0, 0.0], dtype=F64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6), 256.0, 260.0, 0.0], dtype=F64)
    assert torch.equal(rn_bf16(ties), want)
    # a value a hair above a tie must go up although fp32 would first round it onto the tie (the reason rn_bf16 works in fp64)
    assert float(rn_bf16(torch.tensor(1.0 + 2.0 ** -8 + 2.0 ** -40, dtype=F64))) == 1.0 + 2.0 ** -7


@pytest.mark.parametrize("shape", [(2, 24, 5, 7), (3, 56, 4, 3)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_backward_reference_equals_fp64_autograd(shape, act):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(10 + act)
    z = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(BF)
    dy = torch.randn(shape, generator=g).to(BF)
    gamma = (torch.rand(c, generator=g, dtype=F64) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
    beta = torch.randn(c, generator=g, dtype=F64) * 0.5
    slope = torch.tensor([0.1875], dtype=F64)
    x = z.double().requires_grad_(True)
    gm, bt, sl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True), slope.clone().requires_grad_(True)
    u = F.batch_norm(x, None, None, gm, bt, True, 0.1, EPS)
    y = F.prelu(u, sl) if act == 1 else (F.mish(u) if act == 2 else u)
    (y * dy.double()).sum().backward()
    # the batch statistics autograd used, as the arrays the kernel is given (fp64 here, so that both sides compute the same function)
    mean = z.double().mean((0, 2, 3))
    var = z.double().var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()     # noqa: E731
    r = bn_act_bwd_ref(nhwc(z), nhwc(dy), mean, invstd, scale, shift, act, slope)
    assert r.M == n * h * w
    assert _close(r.dz64, nhwc(x.grad))
    assert _close(r.s2, gm.grad) and _close(r.s1, bt.grad)
    if act == 1:
        assert _close(r.s3.reshape(1), sl.grad)
    else:
        assert float(r.s3) == 0.0
    assert bool((r.a1 >= r.s1.abs()).all()) and bool((r.a2 >= r.s2.abs() * (1 - 1e-12)).all()) and float(r.a3) >= abs(float(r.s3))
    assert torch.equal(r.dz.double(), rn_bf16(r.dz64))
    # sums handed in replace the data's own
    r2 = bn_act_bwd_ref(nhwc(z), nhwc(dy), mean, invstd, scale, shift, act, slope, sums=(r.s1, r.s2))
    assert torch.equal(r2.dz64, r.dz64)
    r3 = bn_act_bwd_ref(nhwc(z), nhwc(dy), mean, invstd, scale, shift, act, slope, sums=(r.s1 + 1.0, r.s2))
    assert _close(r3.dz64, r.dz64 - scale / r.M, 1e-9)


def test_backward_reference_bias_form_and_the_sign_convention_at_zero():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 3, 4, 8, generator=g).to(BF)
    dy = torch.randn(1, 3, 4, 8, generator=g).to(BF)
    r = bn_act_bwd_ref(z, dy, None, None, None, None, 0)
    assert r.dz is None and torch.equal(r.s1, dy.double().reshape(-1, 8).sum(0))
    # u == 0 belongs to the slope side: g = dy * slope there, and dy * u = 0 adds nothing to s3
    one, zero = torch.ones(8), torch.zeros(8)
    zz = torch.zeros(1, 1, 1, 8, dtype=BF)
    dd = torch.full((1, 1, 1, 8), 2.0, dtype=BF)
    r = bn_act_bwd_ref(zz, dd, zero, one, one, zero, 1, torch.tensor([0.25]))
    assert torch.equal(r.g, torch.full((1, 8), 0.5, dtype=F64)) and float(r.s3) == 0.0
    y, o, u = bn_act_fwd_ref(torch.tensor([[-2.0, 0.0, 2.0, -0.0, 1.0, -1.0, 4.0, -4.0]], dtype=BF), one, zero, 1, torch.tensor([0.25]))
    assert torch.equal(y.float(), torch.tensor([[-0.5, 0.0, 2.0, 0.0, 1.0, -0.25, 4.0, -1.0]]))


def test_forward_reference_rounds_twice_on_planted_ties():
    e8, e7, e6 = 2.0 ** -8, 2.0 ** -7, 2.0 ** -6
    # (z, scale, shift, res) -> o, y
    rows = [(1.0, 1.0, e8, 0.0, 1.0, 1.0),                     # u = 1 + 2^-8: tie, down to the even 1
            (1.0 + e7, 1.0, e8, 0.0, 1.0 + e6, 1.0 + e6),      # u = 1 + 3 * 2^-8: tie, up to the even 1 + 2^-6
            (-1.0, 1.0, -e8, 0.0, -1.0, -1.0),
            (1.0, 1.0, 0.0, e8, 1.0, 1.0),                     # the tie in the second rounding
            (1.0 + e7, 1.0, 0.0, e8, 1.0 + e7, 1.0 + e6),
            (1.0, 1.0, e8, e8, 1.0, 1.0),                      # ONE rounding of 1 + 2^-8 + 2^-8 would give 1 + 2^-7
            (1.5, 0.5, 0.25, -1.0, 1.0, 0.0),
            (3.0, 1.0 + e7, 0.0, 0.0, 3.03125, 3.03125)]       # 3 * (1 + 2^-7) = 3.0234375: a tie between 3.015625 and 3.03125 (even)
    t = torch.tensor(rows, dtype=F64)
    z, scale, shift, res = (t[:, k].to(BF).reshape(1, -1) for k in range(4))
    assert torch.equal(torch.stack([z, scale, shift, res], -1).double().reshape(-1, 4), t[:, :4])       # all bf16-representable
    y, o, u = bn_act_fwd_ref(z, scale.float().reshape(-1), shift.float().reshape(-1), 0, None, res)
    assert torch.equal(o.reshape(-1), t[:, 4]) and torch.equal(y.double().reshape(-1), t[:, 5])
    assert float(rn_bf16(u + res.double())[0, 5]) == 1.0 + e7                                   # what a single rounding would store
    # Mish: o is the rounded fp64 value of u * tanh(softplus(u))
    y, o, u = bn_act_fwd_ref(z, scale.float().reshape(-1), shift.float().reshape(-1), 2)
    assert torch.equal(o, rn_bf16(F.mish(u))) and torch.equal(y.double(), o)


@pytest.mark.parametrize("rows,cpad", [(1, 8), (5, 16)])
def test_finalize_reference_equals_batchnorm2d(rows, cpad):
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 4, 8, 5, 5
    x = torch.randn(n, c, h, w, generator=g, dtype=F64) * 2.0 + torch.randn(1, c, 1, 1, generator=g, dtype=F64)
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g, dtype=F64))
        bn.bias.copy_(torch.randn(c, generator=g, dtype=F64))
        bn.running_mean.copy_(torch.randn(c, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(c, generator=g, dtype=F64) + 0.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    flat = x.permute(0, 2, 3, 1).reshape(-1, c)
    count = flat.shape[0]
    part = torch.full((rows, 2, cpad), 1e9, dtype=F64)              # channels >= C hold junk the reference must not read
    for r, chunk in enumerate(torch.tensor_split(flat, rows)):
        part[r, 0, :c], part[r, 1, :c] = chunk.sum(0), (chunk * chunk).sum(0)
    bn.train()
    with torch.no_grad():
        y = bn(x)
    mean, invstd, scale, shift, nrm, nrv = bn_finalize_ref(part, c, count, EPS, 0.1, bn.weight.detach(), bn.bias.detach(), rm, rv)
    # eps and momentum reach the C ABI as fp32 values: 1e-5 and 0.1 move by 1e-8 relative
    assert _close(mean, flat.mean(0), 1e-9) and _close(invstd, 1.0 / torch.sqrt(flat.var(0, unbiased=False) + EPS), 1e-7)
    assert _close(nrm, bn.running_mean, 1e-7) and _close(nrv, bn.running_var, 1e-7)
    assert _close(flat * scale + shift, y.permute(0, 2, 3, 1).reshape(-1, c), 1e-7)
    out = bn_finalize_ref(part, c, count, EPS, 0.1, bn.weight.detach(), bn.bias.detach())
    assert out[4] is None and out[5] is None and torch.equal(out[0], mean)


def test_finalize_reference_edges():
    one = torch.ones(8, dtype=F64)
    part = torch.zeros(1, 2, 8, dtype=F64)
    part[0, 0], part[0, 1] = 3.0, 9.0                            # one sample of value 3
    mean, invstd, scale, shift, nrm, nrv = bn_finalize_ref(part, 8, 1, EPS, 0.1, one, 0 * one, 0 * one, one)
    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    assert torch.equal(mean, 3 * one) and _close(invstd, one / eps32 ** 0.5, 1e-14)
    assert _close(nrv, 0.9 * one, 1e-7)                          # count == 1: the biased variance (0) goes into the running estimate
    part[0, 1] = 9.0 - 1e-9                                      # q/count a hair below mu^2: clamped, not a NaN
    assert _close(bn_finalize_ref(part, 8, 1, EPS, 0.1, one, 0 * one)[1], one / eps32 ** 0.5, 1e-14)


def test_upsample_and_pgrad_references():
    g = torch.Generator().manual_seed(6)
    dy = (torch.randint(-4095, 4096, (2, 6, 4, 8), generator=g).float() / 64).to(BF)
    want = F.avg_pool2d(dy.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 4
    assert torch.equal(upsample2x_bwd_ref(dy).double(), rn_bf16(want))
    old = torch.ones(2, 3, 2, 8, dtype=BF)
    assert torch.equal(upsample2x_bwd_ref(dy, old).double(), rn_bf16(want + 1.0))
    p = torch.randn(2, 3, 4, 5, 7, generator=g)
    o = pgrad_to_nhwc_ref(p)
    assert o.shape == (2, 4, 5, 21) and o.dtype == BF
    assert torch.equal(o[1, 2, 3, 2 * 7 + 4], p[1, 2, 2, 3, 4].to(BF)) and torch.equal(o[0, 0, 4, 6], p[0, 0, 0, 4, 6].to(BF))
