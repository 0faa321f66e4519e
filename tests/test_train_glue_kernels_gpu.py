"""GPU tier: the training-path glue kernels of csrc/train.hip -- ryolo_bn_finalize, ryolo_bn_act_fwd, ryolo_bn_act_bwd (BatchNorm and
bias form), ryolo_bn_act_bwd_reduced, ryolo_upsample2x_bwd, ryolo_pgrad_to_nhwc -- each called directly and compared with the plain fp64
references of tests/train_glue_reference.py.

Every bf16 tensor argument is a channel slice (element offset 8, pixel stride > C) of a poisoned buffer with a guard tail, as the training
engine hands these kernels slices of its route / concat buffers; poison and guard must be bit-intact afterwards and inputs bit-unchanged.

Inputs of the BatchNorm passes: z lies on a 2^-6 grid below 4, scale and shift on a 2^-5 grid up to 2 (all bf16-representable), so
u = z*scale + shift is a multiple of 2^-11 below 16: exact in fp32 with or without FMA contraction.  The sign of u therefore cannot differ
between a kernel and the reference, a few planted elements have u == 0 exactly (the slope applies where u <= 0), and no element is left out
of any comparison.  mean / invstd are arbitrary fp32 arrays: kernel and reference evaluate the same formula in the arrays they are given.

Bars (derived from the arithmetic, not from any output).  L = the longest sequential fp32 addition chain of the backward's sums, from
ryolo_bn_act_bwd_bias_order: ceil(slab_pixels / pixel_lanes) [a pixel lane's walk] + pixel_lanes [the block reduce] + ceil(nslab / 32) +
32 [the finalise], + 64 for dslope [lane-strided channels, then the butterfly]; for hand-made partial rows the row count.
  per-channel sums, dslope   |got - (start + ref)| <= (L + 8) * 2^-24 * (A + |start|), A = the fp64 sum of the absolute values of the same
                             terms (the start value is one more term of the chain; 8: the roundings inside a term); Mish + 2^-18 * A (__expf)
  y                          2^-8 * (|o| + |y|) + 2^-20 * (|z*scale| + |shift|), Mish + 2^-18 * |u|
  dz                         2^-8 * |dz| + (L + 16) * 2^-24 * |scale| * (|g| + sum|g| / M + |xhat| * sum|g*xhat| / M)
"""
import ctypes

import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from tests.train_glue_reference import (BF, F64, bn_act_bwd_ref, bn_act_fwd_ref, bn_finalize_ref, pgrad_to_nhwc_ref, upsample2x_bwd_ref)

pytestmark = pytest.mark.gpu

EINVAL = -1               # RYOLO_EINVAL (include/ryolo.h)
POISON = 777.0
OFF, PAD, GUARD = 8, 16, 64   # element offset of a slice, channels behind it, guard pixels behind the last one
I16 = torch.int16
U24, U20, U18, U8 = 2.0 ** -24, 2.0 ** -20, 2.0 ** -18, 2.0 ** -8


def _L():
    from rotate_yolov3_amd import _lib as L
    return L


def _ops():
    from rotate_yolov3_amd.model import hip_train_ops as ops
    return ops


def _pbits():
    return int(torch.tensor(POISON, dtype=BF).view(I16))


class Sl(object):
    """an [n, h, w, c] bf16 tensor at channels off .. off+c of a poisoned [n*h*w + GUARD, cs] buffer on the device"""

    def __init__(self, dev, nhw, c, values=None, off=OFF, cs=None):
        self.nhw = (1, 1, nhw) if isinstance(nhw, int) else tuple(nhw)
        self.npix = self.nhw[0] * self.nhw[1] * self.nhw[2]
        self.c, self.off = c, off
        self.cs = cs if cs is not None else off + c + PAD
        assert off + c <= self.cs
        self.buf = torch.full((self.npix + GUARD, self.cs), POISON, dtype=BF, device=dev)
        self.v = self.buf[:self.npix, off:off + c]                      # [npix, c] view
        if values is not None:
            self.v.copy_(values.reshape(self.npix, c))
        self.t = self.buf[:self.npix].view(*self.nhw, self.cs)[..., off:off + c]
        assert self.t.data_ptr() == self.v.data_ptr() and self.t.stride(2) == self.cs
        self.before = None

    def freeze(self):
        """an input: remember every bit of the buffer"""
        self.before = self.buf.clone()
        return self

    def ptr(self):
        return self.t.data_ptr()

    def poison_intact(self):
        if self.before is not None:
            return torch.equal(self.buf.view(I16), self.before.view(I16))
        b, pb = self.buf.view(I16), _pbits()
        return bool((b[:self.npix, :self.off] == pb).all()) and bool((b[:self.npix, self.off + self.c:] == pb).all()) \
            and bool((b[self.npix:] == pb).all())


def _bits_equal(a, b):
    return a.dtype == b.dtype == BF and a.shape == b.shape and torch.equal(a.contiguous().view(I16), b.contiguous().view(I16))


def _guarded_f32(dev, values):
    """an fp32 array followed by 8 poisoned floats"""
    n = values.numel()
    buf = torch.full((n + 8,), POISON, dtype=torch.float32, device=dev)
    buf[:n] = values
    return buf


def _worst(err, bar):
    """largest err / bar (printed before every assertion, so that a run kept by a script shows the margins)"""
    return float((err / bar.clamp_min(1e-300)).max())


# -------------------------------------------------------------------------------------------------------------- BatchNorm inputs
class Case(object):
    pass


_cases = {}


def _bn_case(dev, npix, C):
    """inputs of one shape, made once on the device and shared by the tests (nothing modifies them: every buffer is frozen)"""
    key = (npix, C)
    if key in _cases:
        return _cases[key]
    k = Case()
    g = torch.Generator(device=dev).manual_seed(1000 * C + npix % 997)
    z = (torch.randn(npix, C, generator=g, device=dev) * 1.25 * 64).round().clamp(-255, 255) / 64       # 2^-6 grid, |z| < 4
    dy = torch.randn(npix, C, generator=g, device=dev)
    res = torch.randn(npix, C, generator=g, device=dev)
    sc = torch.randint(1, 65, (C,), generator=g, device=dev).float() / 32
    sc = sc * torch.where(torch.rand(C, generator=g, device=dev) < 0.4, -1.0, 1.0)                  # 2^-5 grid, 0 < |scale| <= 2
    sh = torch.randint(-64, 65, (C,), generator=g, device=dev).float() / 32
    # planted u == 0: (channel, scale, shift, z) at the first, a middle and the last pixel
    k.plants = [(0, 0.5, -0.5, 1.0), (3, -1.0, 0.75, 0.75), (C - 1, 2.0, -1.0, 0.5)]
    k.plant_pix = sorted(set([0, npix // 2, npix - 1]))
    for ch, s, b, zv in k.plants:
        sc[ch], sh[ch] = s, b
        for p in k.plant_pix:
            z[p, ch] = zv
            dy[p, ch] = 1.5
    k.npix, k.C = npix, C
    k.z, k.dy, k.res = (Sl(dev, npix, C, t.to(BF)).freeze() for t in (z, dy, res))
    k.scale, k.shift = sc, sh
    k.mean = torch.randn(C, generator=g, device=dev) * 0.3
    k.invstd = torch.rand(C, generator=g, device=dev) * 1.5 + 0.5
    k.slope = torch.tensor([0.1], device=dev)                        # backward: an arbitrary fp32 value
    k.slope_fwd = torch.tensor([0.1875], device=dev)                 # forward: u * slope is exact in fp32 too, one rounding in all
    k.f32 = [t.clone() for t in (k.scale, k.shift, k.mean, k.invstd, k.slope, k.slope_fwd)]
    # on the CPU, in fp32: the planted elements really are zeros of u
    zc, scc, shc = k.z.v[k.plant_pix].float().cpu(), sc.cpu(), sh.cpu()
    for ch, _, _, _ in k.plants:
        u = zc[:, ch] * scc[ch] + shc[ch]
        assert u.dtype == torch.float32 and bool((u == 0).all())
    # and u is exact in fp32 everywhere (so its sign is the reference's)
    u32 = k.z.v.float() * sc + sh
    assert torch.equal(u32.double(), k.z.v.double() * sc.double() + sh.double())
    assert int((u32 == 0).sum()) >= len(k.plant_pix)
    if npix * C <= 1 << 22:
        _cases[key] = k
    return k


def _inputs_intact(k):
    now = (k.scale, k.shift, k.mean, k.invstd, k.slope, k.slope_fwd)
    return k.z.poison_intact() and k.dy.poison_intact() and k.res.poison_intact() and all(torch.equal(a, b) for a, b in zip(now, k.f32))


def _chain(npix, C):
    """L of the module docstring, from the library's own description of the reduce pass"""
    sl, npl = ctypes.c_longlong(0), ctypes.c_int(0)
    nslab = _L().lib().ryolo_bn_act_bwd_bias_order(npix, C, ctypes.byref(sl), ctypes.byref(npl))
    assert nslab > 0 and sl.value > 0 and 8 <= npl.value <= 256
    return -(-sl.value // npl.value) + npl.value + -(-nslab // 32) + 32


def test_chain_length_follows_the_slab_geometry():
    """the shapes below sit on the boundaries of the reduce pass: 8 channels have 256 pixel lanes, the slab is 128 pixels up to 131072 pixels
    and 129 from 131073"""
    lib = _L().lib()
    sl, npl = ctypes.c_longlong(0), ctypes.c_int(0)
    for npix, C, want in [(1, 8, (1, 128, 256)), (131072, 8, (1024, 128, 256)), (131073, 8, (1017, 129, 256)), (333, 264, (3, 128, 8)),
                          (250, 56, (2, 128, 64)), (361, 504, (3, 128, 8))]:
        assert (lib.ryolo_bn_act_bwd_bias_order(npix, C, ctypes.byref(sl), ctypes.byref(npl)), sl.value, npl.value) == want
    assert _chain(131073, 8) == 1 + 256 + 32 + 32


# ------------------------------------------------------------------------------------------------------------------- forward
SHAPES = [(1, 8), (100, 8), (127, 24), (128, 24), (129, 24), (250, 56), (300, 56), (333, 264), (131073, 8)]


def _check_fwd(dev, k, act, with_res):
    y = Sl(dev, k.npix, k.C)
    slope = k.slope_fwd if act == 1 else None
    _ops().bn_act_fwd(k.z.t, k.scale, k.shift, act, slope, y.t, residual=k.res.t if with_res else None)
    torch.cuda.synchronize()
    want, o, u = bn_act_fwd_ref(k.z.v, k.scale, k.shift, act, slope, k.res.v if with_res else None)
    bar = U8 * (o.abs() + want.double().abs()) + U20 * ((k.z.v.double() * k.scale.double()).abs() + k.shift.double().abs())
    if act == 2:
        bar = bar + U18 * u.abs()
    err = (y.v.double() - want.double()).abs()
    print("fwd %dx%d act %d res %d: worst err/bar %.3g, %d of %d values differ" %
          (k.npix, k.C, act, with_res, _worst(err, bar), int((err > 0).sum()), err.numel()))
    assert bool((err <= bar).all())
    if act != 2 and not with_res:
        assert _bits_equal(y.v, want)                 # one rounding of an exact fp32 value (u, or u * 0.1875): nothing to tolerate
    assert y.poison_intact() and _inputs_intact(k)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("npix,C", SHAPES)
def test_bn_act_fwd_on_slices(cuda_dev, npix, C, act, with_res):
    _check_fwd(cuda_dev, _bn_case(cuda_dev, npix, C), act, with_res)


# ------------------------------------------------------------------------------------------------------------------ backward
def _starts(dev, C):
    g = torch.Generator(device=dev).manual_seed(77 + C)
    dg = torch.randint(-8, 9, (C,), generator=g, device=dev).float() / 4
    db = torch.randint(-8, 9, (C,), generator=g, device=dev).float() / 4
    return dg, db, torch.tensor([1.25], device=dev)


def _ws(dev, nbytes):
    """a workspace of exactly nbytes inside a larger buffer whose tail is a guard"""
    buf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[:nbytes]


def _param_bars(L, r, act, dg0, db0, ds0):
    mish = U18 if act == 2 else 0.0
    return ((L + 8) * U24 * (r.a2 + dg0.double().abs()) + mish * r.a2,
            (L + 8) * U24 * (r.a1 + db0.double().abs()) + mish * r.a1,
            (L + 64 + 8) * U24 * (r.a3 + ds0.double().abs()))


def _dz_bar(L, r, scale, a1, a2):
    C = scale.numel()
    g, xh = r.g.abs(), r.xhat.abs()
    return (U8 * r.dz64.reshape(-1, C).abs() + (L + 16) * U24 * scale.double().abs() * (g + a1 / r.M + xh * (a2 / r.M)))


def _run_bwd(dev, k, act, give=(True, True, True)):
    """one ryolo_bn_act_bwd call on fresh outputs; returns (dz slice, dgamma, dbeta, dslope buffers with guards, workspace buffer)"""
    dg0, db0, ds0 = _starts(dev, k.C)
    dg, db, ds = _guarded_f32(dev, dg0), _guarded_f32(dev, db0), _guarded_f32(dev, ds0)
    dz = Sl(dev, k.npix, k.C)
    wsbuf, ws = _ws(dev, _ops().bn_bwd_ws_bytes(k.npix, k.C))
    _ops().bn_act_bwd(k.z.t, k.dy.t, (k.mean, k.invstd, k.scale, k.shift), act, k.slope if act == 1 else None, dz.t,
                      dg[:k.C] if give[0] else None, db[:k.C] if give[1] else None, ds[:1] if give[2] else None, ws)
    torch.cuda.synchronize()
    return dz, dg, db, ds, wsbuf


def _check_bwd(dev, k, act, give=(True, True, True)):
    C, L = k.C, _chain(k.npix, k.C)
    dg0, db0, ds0 = _starts(dev, C)
    dz, dg, db, ds, wsbuf = _run_bwd(dev, k, act, give)
    r = bn_act_bwd_ref(k.z.v, k.dy.v, k.mean, k.invstd, k.scale, k.shift, act, k.slope if act == 1 else None)
    bg, bb, bs = _param_bars(L, r, act, dg0, db0, ds0)
    tag = "bwd %dx%d act %d L %d" % (k.npix, C, act, L)
    if give[0]:
        err = (dg[:C].double() - (dg0.double() + r.s2)).abs()
        print("%s: dgamma worst err/bar %.3g" % (tag, _worst(err, bg)))
        assert bool((err <= bg).all())
    else:
        assert torch.equal(dg[:C], dg0)
    if give[1]:
        err = (db[:C].double() - (db0.double() + r.s1)).abs()
        print("%s: dbeta worst err/bar %.3g" % (tag, _worst(err, bb)))
        assert bool((err <= bb).all())
    else:
        assert torch.equal(db[:C], db0)
    if give[2] and act == 1:
        err = (ds[:1].double() - (ds0.double() + r.s3)).abs()
        print("%s: dslope %.9g ref %.9g, err/bar %.3g" % (tag, float(ds[0]), float(ds0.double() + r.s3), _worst(err, bs.reshape(1))))
        assert bool((err <= bs).all())
    else:
        assert torch.equal(ds[:1], ds0)                              # a dslope buffer is bit-unchanged unless the block is PReLU
    bar = _dz_bar(L, r, k.scale, r.a1, r.a2)
    err = (dz.v.double() - r.dz64.reshape(-1, C)).abs()
    print("%s: dz worst err/bar %.3g" % (tag, _worst(err, bar)))
    assert bool((err <= bar).all())
    for buf, n in ((dg, C), (db, C), (ds, 1)):
        assert bool((buf[n:] == POISON).all())
    assert bool((wsbuf[-256:] == 0xA5).all())
    assert dz.poison_intact() and _inputs_intact(k)
    del r, bar, err
    # a second call gives the first one's bits (fixed summation order)
    dz2, dg2, db2, ds2, _ = _run_bwd(dev, k, act, give)
    assert _bits_equal(dz2.v, dz.v) and torch.equal(dg2, dg) and torch.equal(db2, db) and torch.equal(ds2, ds)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("npix,C", SHAPES)
def test_bn_act_bwd_on_slices(cuda_dev, npix, C, act):
    _check_bwd(cuda_dev, _bn_case(cuda_dev, npix, C), act)


@pytest.mark.parametrize("missing", ["dgamma", "dbeta", "dslope"])
def test_bn_act_bwd_optional_parameter_gradients(cuda_dev, missing):
    give = tuple(n != missing for n in ("dgamma", "dbeta", "dslope"))
    _check_bwd(cuda_dev, _bn_case(cuda_dev, 129, 24), 1, give)


@pytest.mark.parametrize("npix,C,what", [(150001, 56, "generic apply body, several trips"),
                                         (5 * 131072 + 37, 64, "fixed-chunk apply body: unrolled loop and tail, default loads"),
                                         (2 * 131072 + 37, 64, "fixed-chunk apply body: the tail loop alone, three trips"),
                                         ((1 << 19) + 13, 128, "non-temporal forward / reduce / apply, forward's second grid-stride trip")])
def test_bn_act_large_shapes(cuda_dev, npix, C, what):
    """act 1 with residual, forward and backward, at the sizes where the passes take their other paths: the apply kernel's grid is 4096
    blocks of 256 threads (more than 2^20 16-byte chunks: several trips; more than 3 * 2^20: the four-pixel loop, then its tail -- one
    trip of it at 5 * 2^20 chunks, which is why the 2 * 2^20 case is here as well: no four-pixel trip, up to three of the tail), the
    forward's 32768 blocks, and tensors of 128 MiB take the non-temporal instantiations.  References on the device."""
    chunks = npix * (C // 8)
    if C == 56:
        assert chunks > 4096 * 256 and (4096 * 256) % 7 != 0
    elif C == 64:
        assert (4 if npix > 1 << 19 else 2) * 4096 * 256 < chunks < (8 if npix > 1 << 19 else 3) * 4096 * 256 and npix * C * 2 < 128 << 20
    else:
        assert npix * C * 2 >= 128 << 20 and chunks > 32768 * 256
    try:
        k = _bn_case(cuda_dev, npix, C)
        _check_fwd(cuda_dev, k, 1, True)
        _check_bwd(cuda_dev, k, 1)
    finally:
        k = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("npix,C", [(361, 504), (129, 8)])
def test_bias_form_accumulates_dbias(cuda_dev, npix, C):
    """stats = None, dz = None (a bias conv in front of a yolo layer): dbias += the per-channel sum of dy, nothing else is written"""
    dev, k = cuda_dev, _bn_case(cuda_dev, npix, C)
    L = _chain(npix, C)
    _, db0, ds0 = _starts(dev, C)
    r = bn_act_bwd_ref(k.z.v, k.dy.v, None, None, None, None, 0)
    bar = (L + 8) * U24 * (r.a1 + db0.double().abs())
    outs = []
    for _ in range(2):
        db, ds = _guarded_f32(dev, db0), _guarded_f32(dev, ds0)
        wsbuf, ws = _ws(dev, _ops().bn_bwd_ws_bytes(npix, C))
        _ops().bn_act_bwd(k.z.t, k.dy.t, None, 0, None, None, None, db[:C], ds[:1], ws)
        torch.cuda.synchronize()
        outs.append(db)
        assert torch.equal(ds[:1], ds0) and bool((db[C:] == POISON).all()) and bool((wsbuf[-256:] == 0xA5).all())
    err = (outs[0][:C].double() - (db0.double() + r.s1)).abs()
    print("bias form %dx%d L %d: dbias worst err/bar %.3g" % (npix, C, L, _worst(err, bar)))
    assert bool((err <= bar).all())
    assert torch.equal(outs[0], outs[1]) and _inputs_intact(k)


# ------------------------------------------------------------------------------------- bn_act_bwd_reduced on hand-made rows
@pytest.mark.parametrize("rows,fold_ws", [(1, True), (2047, True), (2048, True), (2100, True), (4097, True), (2100, False), (4097, False)])
def test_bn_act_bwd_reduced_on_hand_made_rows(cuda_dev, rows, fold_ws):
    """finalise + apply on partial rows the test controls: below 2048 rows the finalise kernel walks them, from 2048 on they are first
    folded to 64 rows when the workspace has room for those (3 + 192) * C floats, and walked as they are when it has 3 * C floats only"""
    dev, C, npix, act = cuda_dev, 64, 200, 1
    k = _bn_case(dev, npix, C)
    g = torch.Generator(device=dev).manual_seed(rows)
    part = torch.randn(rows, 3, C, generator=g, device=dev) * (4.0 / rows ** 0.5)
    part0 = part.clone()
    s = part.double().sum(0)
    a = part.double().abs().sum(0)
    dg0, db0, ds0 = _starts(dev, C)
    r = bn_act_bwd_ref(k.z.v, k.dy.v, k.mean, k.invstd, k.scale, k.shift, act, k.slope, sums=(s[0], s[1]))
    L = rows                                                         # no chain through the rows is longer than the rows
    outs = []
    for _ in range(2):
        dg, db, ds = _guarded_f32(dev, dg0), _guarded_f32(dev, db0), _guarded_f32(dev, ds0)
        dz = Sl(dev, npix, C)
        wsbuf, ws = _ws(dev, (3 + 3 * 64) * C * 4 if fold_ws else 3 * C * 4)
        _ops().bn_act_bwd_reduced(k.z.t, k.dy.t, (k.mean, k.invstd, k.scale, k.shift), act, k.slope, dz.t, dg[:C], db[:C], ds[:1], part, ws)
        torch.cuda.synchronize()
        assert bool((wsbuf[-256:] == 0xA5).all()) and dz.poison_intact() and torch.equal(part, part0)
        outs.append((dz, dg, db, ds))
    dz, dg, db, ds = outs[0]
    for name, got, start, ref, A, Lx in (("dgamma", dg[:C], dg0, s[1], a[1], L), ("dbeta", db[:C], db0, s[0], a[0], L),
                                         ("dslope", ds[:1], ds0, s[2].sum().reshape(1), a[2].sum().reshape(1), L + 64)):
        err = (got.double() - (start.double() + ref)).abs()
        bar = (Lx + 8) * U24 * (A + start.double().abs())
        print("reduced rows %d fold_ws %d: %s worst err/bar %.3g" % (rows, fold_ws, name, _worst(err, bar)))
        assert bool((err <= bar).all())
    bar = _dz_bar(L, r, k.scale, a[0], a[1])
    err = (dz.v.double() - r.dz64.reshape(-1, C)).abs()
    print("reduced rows %d fold_ws %d: dz worst err/bar %.3g" % (rows, fold_ws, _worst(err, bar)))
    assert bool((err <= bar).all())
    for x, y in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(x, y)
    assert _bits_equal(outs[0][0].v, outs[1][0].v) and _inputs_intact(k)


# --------------------------------------------------------------------------------------------------------------- bn_finalize
JUNK = 12345.678


def _finalize_part(R, C, cpad, count, g):
    """fp64 [R, 2, cpad] rows whose sums give per-channel mean m and variance v; channel 1: sum of squares / count a hair BELOW mean^2
    (the clamp); channel 2: |mean| = 1000 standard deviations; channels >= C: junk that must be neither read nor written"""
    m = torch.randn(C, generator=g, dtype=F64) * 2.0
    v = torch.rand(C, generator=g, dtype=F64) * 4.0 + 0.05
    m[1], m[2], v[2] = 1.5, -100.0, 0.01
    s, q = count * m, count * (v + m * m)
    q[1] = count * m[1] * m[1] * (1.0 - 1e-12)
    w = torch.rand(R, generator=g, dtype=F64) + 0.1
    w = w / w.sum()
    part = torch.full((R, 2, cpad), JUNK, dtype=F64)
    part[:, 0, :C] = w[:, None] * s[None, :]
    part[:, 1, :C] = w[:, None] * q[None, :]
    return part


@pytest.mark.parametrize("C,cpad", [(8, 8), (24, 32), (33, 64)])
@pytest.mark.parametrize("R", [1, 31, 33, 256, 257, 600])
def test_bn_finalize_on_hand_made_rows(cuda_dev, R, C, cpad):
    """mean, invstd, scale, shift and the running statistics against the fp64 reference at rtol 1e-6 (fp32 outputs of fp64 sums); the
    scratch holds zeros over channels [0, C) afterwards and its other channels are bit-unchanged (include/ryolo.h).
    shift = beta - mean*scale and running_mean = (1-m)*old + m*mean are DIFFERENCES the kernel forms in fp32 from fp32 factors: on top of
    rtol 1e-6 of the result they get 4 * 2^-24 of the subtracted term (its three roundings and invstd's), which rtol 1e-6 of the result
    covers by itself unless the two terms cancel."""
    dev, eps, mom = cuda_dev, 1e-5, 0.1
    g = torch.Generator().manual_seed(R * 100 + C)
    gamma = torch.randn(C, generator=g) + 0.2
    beta = torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    for count in (1, 7, 92416):
        part = _finalize_part(R, C, cpad, count, g)
        for running in (True, False):
            want = bn_finalize_ref(part, C, count, eps, mom, gamma, beta, rm0 if running else None, rv0 if running else None)
            assert float(want[1][1]) == float(1.0 / torch.sqrt(torch.tensor(eps, dtype=torch.float32).double()))    # the clamp channel
            assert abs(float(want[0][2] * want[1][2])) > 990.0                                                  # |mean| = 1e3 std
            pd = part.to(dev)
            outs = [_guarded_f32(dev, torch.full((C,), POISON)) for _ in range(4)]
            rm, rv = _guarded_f32(dev, rm0), _guarded_f32(dev, rv0)
            gd, bd = gamma.to(dev), beta.to(dev)
            _ops().bn_finalize(pd, C, count, gd, bd, eps, mom, rm[:C] if running else None, rv[:C] if running else None,
                               out=[o[:C] for o in outs])
            torch.cuda.synchronize()
            sub = [None, None, None, 4 * U24 * (want[0] * want[2]).abs()]
            for name, got, ref, extra in zip(("mean", "invstd", "scale", "shift"), outs, want[:4], sub):
                err = (got[:C].cpu().double() - ref).abs()
                bar = 1e-6 * ref.abs() + (extra if extra is not None else 0.0)
                print("finalize R %d C %d count %d: %s worst err/bar %.3g" % (R, C, count, name, _worst(err, bar)))
                assert bool((err <= bar).all()) and bool((got[C:] == POISON).all())
            if running:
                err = (rm[:C].cpu().double() - want[4]).abs()
                assert bool((err <= 1e-6 * want[4].abs() + 4 * U24 * (rm0.double().abs() + want[0].abs())).all())
                err = (rv[:C].cpu().double() - want[5]).abs()
                assert bool((err <= 1e-6 * want[5].abs()).all())
            else:
                assert torch.equal(rm[:C].cpu(), rm0) and torch.equal(rv[:C].cpu(), rv0)
            assert bool((rm[C:] == POISON).all()) and bool((rv[C:] == POISON).all())
            after = pd.cpu()
            assert bool((after[:, :, :C] == 0).all())
            assert torch.equal(after[:, :, C:].contiguous().view(torch.int64), part[:, :, C:].contiguous().view(torch.int64))
            assert torch.equal(gd.cpu(), gamma) and torch.equal(bd.cpu(), beta)


# ------------------------------------------------------------------------------------------------------------ upsample2x_bwd
def _grid_values(shape, g):
    """bf16 values that are multiples of 2^-6 below 64 (an 8-bit integer times 2^-2 .. 2^-6): fp32 sums of five of them are exact"""
    k = torch.randint(-255, 256, shape, generator=g).float()
    e = torch.randint(2, 7, shape, generator=g).float()
    v = k * torch.exp2(-e)
    assert bool((v.abs() < 64).all()) and torch.equal(v.to(BF).float(), v) and torch.equal((v * 64).round(), v * 64)
    return v.to(BF)


# the 2x2 block (a, b, c, d) -> its bf16 sum: exact halves between two bf16 values go to the even neighbour, in both directions
TIES = [((32.0, 32.0, 32.0, 32.5), 128.0), ((32.0, 32.0, 32.0, 33.5), 130.0), ((-32.0, -32.0, -32.0, -32.5), -128.0),
        ((-32.0, -32.0, -32.0, -33.5), -130.0), ((1.0, 1.0, 1.0, 1.015625), 4.0), ((1.0, 1.0, 1.0, 1.046875), 4.0625)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", [(2, 5, 7, 24), (1, 1, 1, 8)])
def test_upsample2x_bwd_exact_on_slices(cuda_dev, shape, accumulate):
    """dx (+)= the sum of each 2x2 block of dy, bit for bit: the inputs make every fp32 sum exact, so the one rounding to bf16 is all there
    is; planted blocks sum to round-to-even ties in both directions"""
    dev = cuda_dev
    n, h, w, c = shape
    g = torch.Generator().manual_seed(11 + c)
    dy = _grid_values((n, 2 * h, 2 * w, c), g)
    old = _grid_values(shape, g)
    for ch, (blk, _) in enumerate(TIES):                              # pixel (0, 0, 0), channels 0 .. 5
        dy[0, 0, 0, ch], dy[0, 0, 1, ch], dy[0, 1, 0, ch], dy[0, 1, 1, ch] = blk
        old[0, 0, 0, ch] = 0.0
    want = upsample2x_bwd_ref(dy, old if accumulate else None)
    for ch, (_, s) in enumerate(TIES):
        assert float(want[0, 0, 0, ch]) == s                          # the reference rounds the ties as stated
    tdy = Sl(dev, (n, 2 * h, 2 * w), c, dy).freeze()
    tdx = Sl(dev, (n, h, w), c, old)
    _ops().upsample2x_bwd(tdy.t, tdx.t, accumulate)
    torch.cuda.synchronize()
    assert _bits_equal(tdx.t.cpu(), want)
    assert tdx.poison_intact() and tdy.poison_intact()


def test_upsample2x_bwd_second_trip_of_the_grid_stride_loop(cuda_dev):
    """dx of 2^23 + 5 pixels x 8 channels: more 16-byte chunks than the 32768 * 256 threads of the largest grid, so some threads take a
    second trip.  Values on a 2^-3 grid below 32 (exact fp32 sums), made and compared on the device, accumulating onto a non-zero dx."""
    dev, W, c = cuda_dev, (1 << 23) + 5, 8
    assert W * (c // 8) > 32768 * 256
    g = torch.Generator(device=dev).manual_seed(12)
    try:
        dy = (torch.randint(-255, 256, (1, 2, 2 * W, c), generator=g, device=dev, dtype=I16).to(BF) * 0.125)
        dx = (torch.randint(-255, 256, (1, 1, W, c), generator=g, device=dev, dtype=I16).to(BF) * 0.125)
        want = upsample2x_bwd_ref(dy, dx)
        _ops().upsample2x_bwd(dy, dx, 1)
        torch.cuda.synchronize()
        assert _bits_equal(dx[:, :, -77:], want[:, :, -77:])          # the pixels only a second trip reaches, so that a failure says where
        assert torch.equal(dx.view(I16), want.view(I16))
    finally:
        dy = dx = want = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- pgrad_to_nhwc
@pytest.mark.parametrize("name,na,no,off,cs", [("tiled", 3, 168, 8, None),
                                               ("generic_output_not_16_byte_aligned", 3, 168, 4, 520),
                                               ("generic_channels_no_multiple_of_8", 3, 7, 8, None),
                                               ("generic_tile_exceeds_lds", 3, 344, 8, None),
                                               ("generic_stride_no_multiple_of_8", 3, 8, 8, 36)])
def test_pgrad_to_nhwc_bitwise_on_every_side_of_the_kernel_choice(cuda_dev, name, na, no, off, cs):
    """fp32 [bs, na, ny, nx, no] -> bf16 NHWC, channel a*no + k, each value rounded once.  The tiled kernel serves 16-byte aligned outputs
    whose channel count and stride are multiples of 8 and whose 32-pixel tile fits 64 KiB of LDS; everything else takes the generic one.
    105 pixels in 3 images of 35: a 32-pixel tile spans two images and the last tile is ragged.  Channels of the buffer outside
    [off, off + na*no) -- the padding channels of the engine's head gradient among them -- keep their poison."""
    dev, bs, ny, nx = cuda_dev, 3, 5, 7
    g = torch.Generator().manual_seed(13 + no)
    p = torch.randn(bs, na, ny, nx, no, generator=g)
    flat = p.view(-1)
    flat[:6] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0])
    want = pgrad_to_nhwc_ref(p)
    assert want.view(-1)[:5].tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6), 1.0 + 2.0 ** -7]
    out = Sl(dev, (bs, ny, nx), na * no, off=off, cs=cs)
    assert (out.ptr() % 16 == 0) == (off % 8 == 0) and (name != "tiled" or (out.cs % 8 == 0 and 32 * na * no * 2 <= 65536))
    pd = p.to(dev)
    _ops().pgrad_to_nhwc(pd, out.t)
    torch.cuda.synchronize()
    assert _bits_equal(out.t.cpu(), want)
    assert out.poison_intact() and torch.equal(pd.cpu(), p)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_einval_and_touch_nothing(cuda_dev):
    """bad channel counts, strides, activations, NULL required pointers, short workspaces: RYOLO_EINVAL before any launch.
    (res_cstride: ryolo_bn_act_fwd validated z_cstride and y_cstride but not the residual's, which it reads with the same 16-byte loads --
    the check was added with this test.)"""
    L = _L()
    lib, dev, st = L.lib(), cuda_dev, L.stream_ptr(cuda_dev)
    npix, C = 16, 8
    g = torch.Generator(device=dev).manual_seed(14)
    z, dy, res, y, dz = (Sl(dev, npix, C, torch.randn(npix, C, generator=g, device=dev).to(BF)) for _ in range(5))
    CS = z.cs
    f = [torch.rand(C, generator=g, device=dev) + 0.5 for _ in range(9)]
    scale, shift, mean, invstd, dgamma, dbeta, gamma, beta, rmean = (t.data_ptr() for t in f)
    slope_t = torch.tensor([0.1, 1.25], device=dev)
    slope, dslope = slope_t.data_ptr(), slope_t.data_ptr() + 4
    wsb = lib.ryolo_bn_act_bwd_workspace_bytes(npix, C)
    ws_t = torch.full((wsb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    ws = ws_t.data_ptr()
    part = torch.randn(4, 3, C, generator=g, device=dev)
    stat = torch.rand(4, 2, C, generator=g, device=dev, dtype=F64)
    up_dy = Sl(dev, (1, 8, 8), C, torch.randn(64, C, generator=g, device=dev).to(BF))
    pg = torch.randn(1, 3, 4, 4, 8, generator=g, device=dev)
    pout = Sl(dev, (1, 4, 4), 24)
    keep = [z, dy, res, y, dz, up_dy, pout]
    tensors = f + [slope_t, ws_t, part, stat, pg]
    snap = [s.buf.clone() for s in keep] + [t.clone() for t in tensors]

    def fwd(z_=z.ptr(), zcs=CS, sc=scale, sh=shift, act=1, res_=res.ptr(), rcs=CS, y_=y.ptr(), ycs=CS, c=C):
        return lib.ryolo_bn_act_fwd(z_, zcs, sc, sh, act, slope, res_, rcs, y_, ycs, npix, c, st)

    def bwd(z_=z.ptr(), zcs=CS, dy_=dy.ptr(), dycs=CS, sc=scale, sh=shift, mu=mean, isd=invstd, act=1, dz_=dz.ptr(), dzcs=CS, c=C, ws_=ws,
            wsbytes=wsb):
        return lib.ryolo_bn_act_bwd(z_, zcs, dy_, dycs, sc, sh, mu, isd, act, slope, dz_, dzcs, npix, c, dgamma, dbeta, dslope, ws_, wsbytes, st)

    def red(part_=part.data_ptr(), rows=4, act=1, wsbytes=3 * C * 4, c=C, dzcs=CS):
        return lib.ryolo_bn_act_bwd_reduced(z.ptr(), CS, dy.ptr(), CS, scale, shift, mean, invstd, act, slope, dz.ptr(), dzcs, npix, c,
                                            dgamma, dbeta, dslope, part_, rows, ws, wsbytes, st)

    def fin(p=stat.data_ptr(), rows=4, c=C, count=16, ga=gamma, be=beta, o=(mean, invstd, scale, shift)):
        return lib.ryolo_bn_finalize(p, rows, C, c, count, 1e-5, 0.1, ga, be, o[0], o[1], o[2], o[3], rmean, rmean, st)

    def ups(dy_=up_dy.ptr(), dycs=CS, dx_=z.ptr(), dxcs=CS, c=C):
        return lib.ryolo_upsample2x_bwd(dy_, dycs, dx_, dxcs, 1, 4, 4, c, 1, st)

    def pgr(p=pg.data_ptr(), o=pout.ptr(), ocs=pout.cs):
        return lib.ryolo_pgrad_to_nhwc(p, 1, 3, 4, 4, 8, o, ocs, st)

    calls = {
        "fwd C": lambda: fwd(c=12), "fwd z_cstride": lambda: fwd(zcs=CS + 4), "fwd y_cstride": lambda: fwd(ycs=CS + 4),
        "fwd res_cstride": lambda: fwd(rcs=CS + 4), "fwd act": lambda: fwd(act=3), "fwd act<0": lambda: fwd(act=-1),
        "fwd z": lambda: fwd(z_=None), "fwd scale": lambda: fwd(sc=None), "fwd shift": lambda: fwd(sh=None), "fwd y": lambda: fwd(y_=None),
        "bwd C": lambda: bwd(c=12), "bwd z_cstride": lambda: bwd(zcs=CS + 4), "bwd dy_cstride": lambda: bwd(dycs=CS + 4),
        "bwd dz_cstride": lambda: bwd(dzcs=CS + 4), "bwd act": lambda: bwd(act=3), "bwd z": lambda: bwd(z_=None),
        "bwd dy": lambda: bwd(dy_=None), "bwd workspace": lambda: bwd(ws_=None), "bwd shift": lambda: bwd(sh=None),
        "bwd mean": lambda: bwd(mu=None), "bwd invstd": lambda: bwd(isd=None), "bwd dz": lambda: bwd(dz_=None),
        "bwd workspace one byte short": lambda: bwd(wsbytes=wsb - 1),
        "reduced part": lambda: red(part_=None), "reduced rows": lambda: red(rows=0), "reduced act": lambda: red(act=2),
        "reduced workspace one byte short": lambda: red(wsbytes=3 * C * 4 - 1), "reduced C": lambda: red(c=12),
        "reduced dz_cstride": lambda: red(dzcs=CS + 4),
        "finalize part": lambda: fin(p=None), "finalize rows": lambda: fin(rows=0), "finalize C": lambda: fin(c=0),
        "finalize count": lambda: fin(count=0), "finalize gamma": lambda: fin(ga=None), "finalize beta": lambda: fin(be=None),
        "finalize mean": lambda: fin(o=(None, invstd, scale, shift)), "finalize invstd": lambda: fin(o=(mean, None, scale, shift)),
        "finalize scale": lambda: fin(o=(mean, invstd, None, shift)), "finalize shift": lambda: fin(o=(mean, invstd, scale, None)),
        "upsample C": lambda: ups(c=12), "upsample dy_cstride": lambda: ups(dycs=CS + 4), "upsample dx_cstride": lambda: ups(dxcs=CS + 4),
        "upsample dy": lambda: ups(dy_=None), "upsample dx": lambda: ups(dx_=None),
        "pgrad out_cstride < na*no": lambda: pgr(ocs=23), "pgrad pgrad": lambda: pgr(p=None), "pgrad out": lambda: pgr(o=None),
    }
    assert wsb == lib.ryolo_bn_act_bwd_workspace_bytes(npix, C) == (1 * 3 * C + 3 * C) * 4
    for name, call in calls.items():
        assert call() == EINVAL, name
    torch.cuda.synchronize()
    for a, b in zip([s.buf for s in keep] + tensors, snap):
        assert torch.equal(a.view(torch.uint8) if a.dtype != BF else a.view(I16), b.view(torch.uint8) if b.dtype != BF else b.view(I16))
    # the same calls with good arguments are accepted (the refusals above were about the one argument each names)
    assert fwd() == 0 and bwd() == 0 and red() == 0 and fin() == 0 and ups() == 0 and pgr() == 0
    torch.cuda.synchronize()
