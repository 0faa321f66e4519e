"""Plain fp64 references of the training-path glue kernels (csrc/train.hip), written from their contracts -- the kernel comments and
include/ryolo.h -- in torch without autograd.  Every function takes the STORED inputs (bf16 tensors, fp32 parameter arrays), widens them
to fp64 and evaluates the stated formula there; what a kernel stores as bf16 is rounded once, to nearest even, from the fp64 value.
They run on whatever device their inputs live on (the large GPU cases keep everything on the device).

  BatchNorm block forward   u = z*scale + shift;  o = bf16(act(u));  y = bf16(o + res)            (two roundings, as the kernel's header says)
  BatchNorm block backward  g = dy*act'(u);  s1 = sum g;  s2 = invstd * sum g*(z - mean);  s3 = sum over u <= 0 of dy*u
                            dz = scale * (g - s1/M - xhat*s2/M),  xhat = (z - mean)*invstd;  dgamma += s2, dbeta += s1, dslope += s3
  act                       0 linear, 1 leaky / PReLU (the slope applies where u <= 0), 2 Mish = u * tanh(softplus(u))
"""
import torch

BF = torch.bfloat16
F64 = torch.float64


def rn_bf16(x):
    """fp64 -> the nearest bf16 value (8 significant bits, ties to even), still as fp64.  Normal range only: no overflow to infinity and
    no denormals, which none of the callers reach.  (x.to(bfloat16) is not used: it may round through fp32 first.)"""
    m, e = torch.frexp(x.to(F64))                      # x = m * 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(m * 256.0), e - 8)  # torch.round: halves to even


def _d(t):
    return None if t is None else t.to(F64)


def _mish(u):
    return u * torch.tanh(torch.logaddexp(u, torch.zeros_like(u)))


def _mish_grad(u):
    t = torch.tanh(torch.logaddexp(u, torch.zeros_like(u)))
    return t + u * (1.0 - t * t) * torch.sigmoid(u)


def _slope(slope, like):
    return torch.zeros((), dtype=F64, device=like.device) if slope is None else slope.to(F64).reshape(())


def bn_finalize_ref(part, C, count, eps, momentum, gamma, beta, run_mean=None, run_var=None):
    """part: fp64 [R, 2, cpad] partial sums of z and z^2.  Returns (mean, invstd, scale, shift, new_run_mean, new_run_var) in fp64, the
    running pair None when no running stats are given.  eps and momentum are the fp32 values the C ABI receives."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))    # noqa: E731
    eps, momentum = f32(eps), f32(momentum)
    s = part[:, 0, :C].to(F64).sum(0)
    q = part[:, 1, :C].to(F64).sum(0)
    mu = s / count
    var = (q / count - mu * mu).clamp_min(0.0)                      # biased, clamped at 0
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = _d(gamma) * invstd
    shift = _d(beta) - mu * scale
    if run_mean is None:
        return mu, invstd, scale, shift, None, None
    unb = var * count / (count - 1.0) if count > 1 else var
    return (mu, invstd, scale, shift, (1.0 - momentum) * _d(run_mean) + momentum * mu, (1.0 - momentum) * _d(run_var) + momentum * unb)


def bn_act_fwd_ref(z, scale, shift, act, slope=None, res=None):
    """Returns (y, o, u): y the stored bf16 result, o the (bf16-valued) fp64 activation output before the residual, u = z*scale + shift."""
    u = _d(z) * _d(scale) + _d(shift)
    if act == 1:
        a = torch.where(u <= 0, u * _slope(slope, u), u)
    elif act == 2:
        a = _mish(u)
    else:
        assert act == 0
        a = u
    o = rn_bf16(a)
    y = o if res is None else rn_bf16(o + _d(res))
    return y.to(BF), o, u


class BwdRef(object):
    """dz (bf16) and dz64 (unrounded); g, xhat [M, C]; per-channel s1, s2 and the scalar s3; the sums of absolute values of the same terms
    a1, a2 [C] and a3 (scalar); M"""


def bn_act_bwd_ref(z, dy, mean, invstd, scale, shift, act, slope=None, sums=None):
    """z, dy: bf16 [..., C].  scale None: the bias form (g = dy, only s1 / a1 are meaningful, no dz).  sums = (s1, s2) replaces the sums
    the data gives in dz's formula (ryolo_bn_act_bwd_reduced applies the sums of the partial rows it is handed)."""
    r = BwdRef()
    C = z.shape[-1]
    zf, d = _d(z).reshape(-1, C), _d(dy).reshape(-1, C)
    r.M = M = zf.shape[0]
    zero = torch.zeros((), dtype=F64, device=zf.device)
    if scale is None:
        r.g, r.s1, r.a1 = d, d.sum(0), d.abs().sum(0)
        r.s2 = r.a2 = torch.zeros(C, dtype=F64, device=zf.device)
        r.s3 = r.a3 = zero
        r.dz = r.dz64 = r.xhat = None
        return r
    sc, sh, mu, istd = _d(scale), _d(shift), _d(mean), _d(invstd)
    u = zf * sc + sh
    r.s3 = r.a3 = zero
    if act == 1:
        neg = u <= 0
        g = torch.where(neg, d * _slope(slope, u), d)
        t3 = torch.where(neg, d * u, torch.zeros_like(u))
        r.s3, r.a3 = t3.sum(), t3.abs().sum()
    elif act == 2:
        g = d * _mish_grad(u)
    else:
        assert act == 0
        g = d
    zc = zf - mu
    r.g, r.xhat = g, zc * istd
    r.s1, r.a1 = g.sum(0), g.abs().sum(0)
    r.s2, r.a2 = istd * (g * zc).sum(0), istd.abs() * (g * zc).abs().sum(0)
    s1, s2 = (r.s1, r.s2) if sums is None else (_d(sums[0]), _d(sums[1]))
    r.dz64 = (sc * (g - s1 / M - r.xhat * (s2 / M))).reshape(z.shape)
    r.dz = rn_bf16(r.dz64).to(BF)
    return r


def upsample2x_bwd_ref(dy, dx_old=None):
    """dy: bf16 [N, 2H, 2W, C] -> dx bf16 [N, H, W, C] = bf16(sum of each 2x2 block (+ dx_old)): one rounding of the exact sum"""
    n, h2, w2, c = dy.shape
    s = _d(dy).reshape(n, h2 // 2, 2, w2 // 2, 2, c).sum((2, 4))
    if dx_old is not None:
        s = s + _d(dx_old)
    return rn_bf16(s).to(BF)


def pgrad_to_nhwc_ref(pgrad):
    """fp32 [bs, na, ny, nx, no] -> bf16 [bs, ny, nx, na*no], channel = a*no + k, each value rounded once (fp32 -> bf16 is a single
    round-to-nearest-even in torch)"""
    bs, na, ny, nx, no = pgrad.shape
    return pgrad.permute(0, 2, 3, 1, 4).reshape(bs, ny, nx, na * no).to(BF)
