"""GPU tier: the small NHWC kernels between the conv stack and the decode (csrc/yolo.hip: add, nearest upsample, maxpool) and the two
layout converters at the model boundary (csrc/conv.hip), each called through the C ABI and compared with a plain reference.  All of these
operations are exact (a copy, a maximum, one correctly rounded sum or conversion): every comparison is bit for bit, no tolerance.
Every tensor is a channel slice of a wider poisoned buffer, and the poison must be intact afterwards.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rotate_yolov3_amd  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1               # RYOLO_EINVAL (include/ryolo.h)
POISON = 777.0
OFF, CS = 8, 40           # element offset of the slice and pixel stride of the buffer around it
BF = torch.bfloat16


def _lib():
    from rotate_yolov3_amd import _lib as L
    return L


class Sliced(object):
    """an [N, H, W, C] bf16 tensor living at channels OFF .. OFF+C of a poisoned [N, H, W, CS] buffer on the device"""

    def __init__(self, dev, shape, values=None, cs=CS):
        n, h, w, c = shape
        assert OFF + c <= cs
        buf = torch.full((n, h, w, cs), POISON, dtype=BF)
        if values is not None:
            buf[..., OFF:OFF + c] = values
        self.buf = buf.to(dev)
        self.t = self.buf[..., OFF:OFF + c]
        self.c, self.cs = c, cs

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        return self.t.cpu()

    def poison_intact(self):
        b = self.buf.cpu()
        return bool((b[..., :OFF] == POISON).all()) and bool((b[..., OFF + self.c:] == POISON).all())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.dtype == b.dtype == BF and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


N, H, W, C = 2, 5, 7, 24


# ------------------------------------------------------------------------------------------------------------------------- add
def _add_inputs():
    g = torch.Generator().manual_seed(1)
    a = (torch.randn(N, H, W, C, generator=g) * 4).to(BF)
    b = (torch.randn(N, H, W, C, generator=g) * 4).to(BF)
    # sums that lie exactly half way between two bf16 values (8 significant bits): ties go to the even neighbour, in both directions
    ties = [(1.0, 2.0 ** -8, 1.0),                       # 1 + 2^-8        -> 1          (down)
            (1.0 + 2.0 ** -7, 2.0 ** -8, 1.0 + 2.0 ** -6),   # 1 + 3 * 2^-8    -> 1 + 2^-6   (up)
            (-1.0, -(2.0 ** -8), -1.0),
            (-(1.0 + 2.0 ** -7), -(2.0 ** -8), -(1.0 + 2.0 ** -6)),
            (256.0, 1.0, 256.0),                          # 257 -> 256
            (258.0, 1.0, 260.0),                          # 259 -> 260
            (3.0e38, 3.0e38, float("inf")),               # overflow of the sum
            (0.0, -0.0, 0.0)]
    for k, (x, y, _) in enumerate(ties):
        a[k % N, k % H, (k * 3) % W, (k * 5) % C] = x
        b[k % N, k % H, (k * 3) % W, (k * 5) % C] = y
    want = (a.float() + b.float()).to(BF)
    for k, (_, _, s) in enumerate(ties):
        assert want[k % N, k % H, (k * 3) % W, (k * 5) % C] == s      # the reference itself rounds these as stated
    return a, b, want


@pytest.mark.parametrize("form", ["out_of_place", "y_is_b", "y_is_a"])
def test_add_nhwc_exact_with_rounding_ties_and_in_place_forms(cuda_dev, form):
    """ryolo_add_nhwc == bf16(float(a) + float(b)) bit for bit, ties to even included; y may be exactly one of the inputs (the training
    engine accumulates a shortcut's gradient in place, y == b)"""
    L = _lib()
    a, b, want = _add_inputs()
    ta, tb = Sliced(cuda_dev, (N, H, W, C), a), Sliced(cuda_dev, (N, H, W, C), b)
    ty = {"out_of_place": Sliced(cuda_dev, (N, H, W, C)), "y_is_b": tb, "y_is_a": ta}[form]
    rc = L.lib().ryolo_add_nhwc(ta.ptr(), CS, tb.ptr(), CS, ty.ptr(), CS, N * H * W, C, L.stream_ptr(cuda_dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert _same(ty.cpu(), want)
    assert ta.poison_intact() and tb.poison_intact() and ty.poison_intact()
    if form != "y_is_a":
        assert _same(ta.cpu(), a)
    if form != "y_is_b":
        assert _same(tb.cpu(), b)


# -------------------------------------------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("scale", [1, 2, 3])
def test_upsample_nhwc_equals_nearest_interpolate(cuda_dev, scale):
    L = _lib()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, H, W, C, generator=g).to(BF)
    want = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=scale, mode="nearest").permute(0, 2, 3, 1).to(BF)
    assert want.shape == (N, H * scale, W * scale, C)
    tx, ty = Sliced(cuda_dev, (N, H, W, C), x), Sliced(cuda_dev, (N, H * scale, W * scale, C))
    rc = L.lib().ryolo_upsample_nhwc(tx.ptr(), CS, ty.ptr(), CS, N, H, W, C, scale, L.stream_ptr(cuda_dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert _same(ty.cpu(), want)
    assert ty.poison_intact() and tx.poison_intact() and _same(tx.cpu(), x)


# --------------------------------------------------------------------------------------------------------------------- maxpool
def _maxpool_ref(x_nhwc, k, s):
    """as the reference model builds the layer (model/models.py:79-87): size 2 / stride 1 is ZeroPad2d((0, 1, 0, 1)) + MaxPool2d(2, 1) --
    an explicit zero takes part in the maximum on the right and bottom border; every other size pads (k-1)//2 with -inf"""
    x = x_nhwc.float().permute(0, 3, 1, 2)
    y = F.max_pool2d(F.pad(x, (0, 1, 0, 1)), 2, 1) if (k, s) == (2, 1) else F.max_pool2d(x, k, s, padding=(k - 1) // 2)
    return y.permute(0, 2, 3, 1).to(BF)


@pytest.mark.parametrize("sign", ["signed", "all_negative"])
@pytest.mark.parametrize("hw", [(5, 7), (13, 13)])
@pytest.mark.parametrize("k,s", [(2, 2), (2, 1), (3, 1), (3, 2), (5, 1), (13, 1)])
def test_maxpool_nhwc_equals_the_reference_layer(cuda_dev, k, s, hw, sign):
    """ryolo_maxpool_nhwc at every (size, stride) the cfgs use, on a signed and on an all-negative input: with all inputs negative the
    zero padding of size 2 / stride 1 shows (last row and column are 0), and the -inf padding of every other size must not"""
    L = _lib()
    h, w = hw
    g = torch.Generator().manual_seed(3 + k)
    x = torch.randn(N, h, w, C, generator=g)
    if sign == "all_negative":
        x = -(x.abs() + 0.125)
    x = x.to(BF)
    want = _maxpool_ref(x, k, s)
    ho, wo = want.shape[1:3]
    tx, ty = Sliced(cuda_dev, (N, h, w, C), x), Sliced(cuda_dev, (N, ho, wo, C))
    rc = L.lib().ryolo_maxpool_nhwc(tx.ptr(), CS, ty.ptr(), CS, N, h, w, C, k, s, L.stream_ptr(cuda_dev))
    assert rc == 0
    torch.cuda.synchronize()
    got = ty.cpu()
    assert _same(got, want)
    assert ty.poison_intact() and tx.poison_intact() and _same(tx.cpu(), x)
    if sign == "all_negative":
        if (k, s) == (2, 1):
            assert (ho, wo) == (h, w)
            assert bool((got[:, -1] == 0).all()) and bool((got[:, :, -1] == 0).all()) and bool((got[:, :-1, :-1] < 0).all())
        else:
            assert bool((got < 0).all())


def test_nhwc_helpers_refuse_channel_counts_and_strides_that_are_no_multiple_of_8(cuda_dev):
    L = _lib()
    lib, st = L.lib(), L.stream_ptr(cuda_dev)
    x, y = Sliced(cuda_dev, (N, H, W, C)), Sliced(cuda_dev, (N, 3 * H, 3 * W, C))
    before = y.buf.clone()
    for c, cs in ((20, CS), (C, 36)):
        assert lib.ryolo_add_nhwc(x.ptr(), cs, x.ptr(), cs, y.ptr(), cs, N * H * W, c, st) == EINVAL
        assert lib.ryolo_upsample_nhwc(x.ptr(), cs, y.ptr(), cs, N, H, W, c, 2, st) == EINVAL
        assert lib.ryolo_maxpool_nhwc(x.ptr(), cs, y.ptr(), cs, N, H, W, c, 3, 1, st) == EINVAL
    assert lib.ryolo_add_nhwc(x.ptr(), CS, x.ptr(), 36, y.ptr(), CS, N * H * W, C, st) == EINVAL
    assert lib.ryolo_add_nhwc(x.ptr(), CS, x.ptr(), CS, y.ptr(), 36, N * H * W, C, st) == EINVAL
    assert lib.ryolo_upsample_nhwc(x.ptr(), CS, y.ptr(), 36, N, H, W, C, 2, st) == EINVAL
    assert lib.ryolo_maxpool_nhwc(x.ptr(), CS, y.ptr(), 36, N, H, W, C, 3, 1, st) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(y.buf, before)                     # refused before any launch


# ------------------------------------------------------------------------------------------------------------------ converters
FLT_MAX = float(np.finfo(np.float32).max)
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), 1e-40, -1e-40, FLT_MAX, -FLT_MAX, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
            -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), float("nan")]


@pytest.mark.parametrize("c,cpad", [(3, 8), (3, 16), (8, 8), (8, 16), (11, 16)])
def test_nchw_f32_to_nhwc_bf16_bitwise_with_special_values(cuda_dev, c, cpad):
    """the input converter == x.to(bfloat16) (round to nearest even) bit for bit: signed zeros, infinities, an fp32 denormal, FLT_MAX
    (rounds to inf), ties in both directions; NaN stays NaN; channels C .. Cpad-1 are exact zeros; nothing is written behind the tensor"""
    L = _lib()
    n, h, w = 2, 17, 23
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, c, h, w, generator=g)
    for k, v in enumerate(SPECIALS):
        x[k % n, k % c, (k * 5) % h, (k * 7) % w] = v
        x[(k + 1) % n, c - 1, (k * 3 + 1) % h, (k * 11 + 2) % w] = v          # the last real channel, next to the padding
    want = x.permute(0, 2, 3, 1).to(BF)
    sp = torch.tensor(SPECIALS).to(BF)                        # what the reference makes of them
    assert sp[6] == float("inf") and sp[7] == float("-inf") and sp[8] == 1.0 and sp[9] == 1.0 + 2.0 ** -6 and sp[10] == -1.0
    assert bool((_bits(sp[4:6]) & 0x7fff).eq(1).all())       # 1e-40 is the smallest bf16 denormal, not zero
    assert int((want == float("inf")).sum()) >= 2 and int((_bits(want) & 0x7fff).eq(1).sum()) >= 2 and int(torch.isnan(want).sum()) >= 1
    npix = n * h * w
    xd = x.to(cuda_dev)
    y = torch.full((npix * cpad + 64,), POISON, dtype=BF, device=cuda_dev)
    rc = L.lib().ryolo_nchw_f32_to_nhwc_bf16(xd.data_ptr(), n, c, h, w, cpad, y.data_ptr(), L.stream_ptr(cuda_dev))
    assert rc == 0
    torch.cuda.synchronize()
    y = y.cpu()
    got = y[:npix * cpad].view(n, h, w, cpad)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got[..., :c]), nan)
    assert torch.equal(_bits(got[..., :c])[~nan], _bits(want)[~nan])
    assert bool((_bits(got[..., c:]) == 0).all())             # padding channels: +0, bit for bit
    assert bool((y[npix * cpad:] == POISON).all())
    if cpad < 16:
        assert L.lib().ryolo_nchw_f32_to_nhwc_bf16(xd.data_ptr(), n, 11, h, w, 8, y.data_ptr(), L.stream_ptr(cuda_dev)) == EINVAL   # Cpad < C


@pytest.mark.parametrize("c", [3, 11, 24])
def test_nhwc_bf16_to_nchw_f32_from_a_channel_slice(cuda_dev, c):
    """the output converter reads a slice with pixel stride > C and widens exactly (bf16 denormals, infinities, -0, NaN)"""
    L = _lib()
    n, h, w = 2, 17, 23
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, h, w, c, generator=g).to(BF)
    for k, v in enumerate([0.0, -0.0, float("inf"), float("-inf"), 1e-40, -1e-40, 3.3e38, float("nan")]):
        x[k % n, (k * 5) % h, (k * 7) % w, k % c] = v
        x[(k + 1) % n, (k * 3 + 1) % h, (k * 11 + 2) % w, c - 1] = v
    want = x.float().permute(0, 3, 1, 2).contiguous()
    tx = Sliced(cuda_dev, (n, h, w, c), x)
    y = torch.full((want.numel() + 64,), POISON, dtype=torch.float32, device=cuda_dev)
    rc = L.lib().ryolo_nhwc_bf16_to_nchw_f32(tx.ptr(), n, c, h, w, CS, y.data_ptr(), L.stream_ptr(cuda_dev))
    assert rc == 0
    torch.cuda.synchronize()
    y = y.cpu()
    got = y[:want.numel()].view(n, c, h, w)
    nan = torch.isnan(want)
    assert int(nan.sum()) >= 1 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])
    assert bool((y[want.numel():] == POISON).all()) and tx.poison_intact()


# ------------------------------------------------------------------------------------ the second trip of the grid-stride loops
GRID_CAP = 65536 * 256        # csrc/yolo.hip grid_for(): at most 65536 blocks of 256 threads, one 8-channel group per thread and trip
CONV_CAP = 16384 * 256        # csrc/conv.hip: the converters' grids


@pytest.mark.parametrize("op", ["add", "upsample2", "maxpool2x2", "nchw_to_nhwc", "nhwc_to_nchw"])
def test_second_trip_of_the_grid_stride_loop(cuda_dev, op):
    """the smallest shapes whose work-item count just exceeds the grid cap, so that some threads take a second trip of their loop (the
    real workloads do: the unfused add of the se cfgs at 304^2 x 64 x batch 32, the input converter at 608^2 x batch 32).  Inputs are made
    on the device and the reference is the matching ATen operation on the device -- exact operations; nothing large crosses to the host."""
    L = _lib()
    lib, dev, st = L.lib(), cuda_dev, L.stream_ptr(cuda_dev)
    g = torch.Generator(device=dev).manual_seed(9)
    c = 64
    try:
        if op == "add":
            npix = GRID_CAP // (c // 8) + 77
            assert npix * (c // 8) > GRID_CAP
            a = torch.randn(npix, c, generator=g, device=dev, dtype=BF)
            b = torch.randn(npix, c, generator=g, device=dev, dtype=BF)
            y = torch.empty_like(a)
            assert lib.ryolo_add_nhwc(a.data_ptr(), c, b.data_ptr(), c, y.data_ptr(), c, npix, c, st) == 0
            assert torch.equal(y, torch.add(a, b))
            # the tail alone (the rows only a second trip reaches), so that a failure says where
            assert torch.equal(y[-77:], torch.add(a[-77:], b[-77:]))
        elif op == "upsample2":
            h, w = 725, 724
            assert 4 * h * w * (c // 8) > GRID_CAP
            x = torch.randn(1, h, w, c, generator=g, device=dev, dtype=BF)
            y = torch.empty(1, 2 * h, 2 * w, c, device=dev, dtype=BF)
            assert lib.ryolo_upsample_nhwc(x.data_ptr(), c, y.data_ptr(), c, 1, h, w, c, 2, st) == 0
            want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
            assert torch.equal(y.permute(0, 3, 1, 2), want)
        elif op == "maxpool2x2":
            h, w = 2900, 2896
            assert (h // 2) * (w // 2) * (c // 8) > GRID_CAP
            x = torch.randn(1, h, w, c, generator=g, device=dev, dtype=BF)
            y = torch.empty(1, h // 2, w // 2, c, device=dev, dtype=BF)
            assert lib.ryolo_maxpool_nhwc(x.data_ptr(), c, y.data_ptr(), c, 1, h, w, c, 2, 2, st) == 0
            want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2)
            assert torch.equal(y.permute(0, 3, 1, 2), want)
        elif op == "nchw_to_nhwc":
            n, ch, h, w = 1, 3, 2049, 2048
            assert n * h * w > CONV_CAP
            x = torch.randn(n, ch, h, w, generator=g, device=dev)
            y = torch.empty(n, h, w, 8, device=dev, dtype=BF)
            assert lib.ryolo_nchw_f32_to_nhwc_bf16(x.data_ptr(), n, ch, h, w, 8, y.data_ptr(), st) == 0
            assert torch.equal(y[..., :ch], x.permute(0, 2, 3, 1).to(BF)) and bool((y[..., ch:] == 0).all())
        else:
            n, ch, h, w = 1, 8, 725, 725
            assert n * ch * h * w > CONV_CAP
            x = torch.randn(n, h, w, ch, generator=g, device=dev, dtype=BF)
            y = torch.empty(n, ch, h, w, device=dev)
            assert lib.ryolo_nhwc_bf16_to_nchw_f32(x.data_ptr(), n, ch, h, w, ch, y.data_ptr(), st) == 0
            assert torch.equal(y, x.permute(0, 3, 1, 2).float())
    finally:
        a = b = x = y = want = None
        torch.cuda.empty_cache()
