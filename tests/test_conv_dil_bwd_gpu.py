"""GPU tier of the dilated shared convs' training kernels: ryolo_conv2d_dilated_wgrad (csrc/wgrad_dil.hip) and ryolo_conv2d_dilated_dgrad
(csrc/conv_dil.hip) against fp32 ATen autograd on the CPU on the same bf16-rounded operands (tests/dilated_bwd_reference.py), their
accumulate / slice / reproducibility / refusal contracts, the packed-image equality the data gradient rests on, and the autograd Function
SharedDilatedConv.

Bars: weight gradient max|err| <= 2e-3 max|dW| + 1e-3 (test_wgrad_vs_autograd's); data gradient 2^-7 * sum|terms| + 2e-3 per element (the
dilated forward's: it is the same kernel)."""
import ctypes as C

import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
import oracle
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model import hip_train_ops as T
from tests import dilated_bwd_reference as br

pytestmark = pytest.mark.gpu
torch.set_num_threads(oracle.host_cores(16))

EINVAL = -1
SWEEP = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (1, 4), (8, 1)]
ODD = (2, 9, 7, 64, 64)       # 126 pixels, two images


def _seed(dil):
    return dil[0] * 10 + dil[1]


def _ws(d, dil, dev, fill=None):
    nbytes = T.conv_dilated_wgrad_ws_bytes(d, dil)
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws.view(torch.uint8)


def _wgrad(dev, x, dy, dil, grad=None, accumulate=False, ws_fill=None):
    """x, dy: NHWC bf16 device tensors (possibly slices)"""
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    d = T.dilated_desc(n, h, w, cin, cout, in_cs=x.stride(2), out_cs=dy.stride(2))
    if grad is None:
        grad = torch.full((cout, cin, 3, 3), float("nan"), dtype=torch.float32, device=dev)
    T.conv_dilated_wgrad(d, dil, x, dy, grad, accumulate, _ws(d, dil, dev, ws_fill))
    torch.cuda.synchronize()
    return grad


def _dgrad(dev, dy, wt, dil, cin, dx=None):
    n, h, w, cout = dy.shape
    if dx is None:
        dx = torch.empty((n, h, w, cin), dtype=torch.bfloat16, device=dev)
    d = T.dilated_desc(n, h, w, cin, cout, in_cs=dx.stride(2), out_cs=dy.stride(2))
    packed = T.pack_weights_dgrad(wt.to(dev), 1)
    ones, zeros = torch.ones(ops.cpad(cin), device=dev), torch.zeros(ops.cpad(cin), device=dev)
    T.conv_dilated_dgrad(d, dil, dy, packed, ones, zeros, dx)
    torch.cuda.synchronize()
    return dx


def _wgrad_case(dev, shape, dil, seed):
    r = br.reference(*shape, dil, seed)
    got = _wgrad(dev, r["x"].to(dev), r["dy"].to(dev), dil)
    assert not bool(torch.isnan(got).any())
    br.check_wgrad(got, r["dw"], "N %d %dx%d %d->%d dil %s" % (shape + (dil,)))
    return got, r


# ---------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("dil", SWEEP, ids=lambda d: "d%dx%d" % d)
def test_wgrad_vs_autograd_odd_map_two_images(cuda_dev, dil):
    """126 pixels, below any K chunk's multiple; two images, so a border test on the flat offset would sum image 0's rows into the taps
    above row 0 of image 1"""
    _wgrad_case(cuda_dev, ODD, dil, _seed(dil))


def test_wgrad_several_image_wraps_inside_one_k_step(cuda_dev):
    _wgrad_case(cuda_dev, (5, 3, 4, 64, 128), (1, 2), 21)


@pytest.mark.parametrize("dil", [(4, 1), (1, 2)], ids=lambda d: "d%dx%d" % d)
def test_wgrad_more_than_one_cout_tile_and_split(cuda_dev, dil):
    """432 pixels, 128 -> 256: two C_out tiles of 128 and (18 workgroups per split against a round of 512) one split per 64-pixel K step: 7"""
    d = T.dilated_desc(3, 12, 12, 128, 256)
    per_split = 256 * 9 * 128 * 4
    assert T.conv_dilated_wgrad_ws_bytes(d, dil) == 7 * per_split         # more than one split is reached, not assumed
    _wgrad_case(cuda_dev, (3, 12, 12, 128, 256), dil, 30 + _seed(dil))


def test_wgrad_long_channels(cuda_dev):
    _wgrad_case(cuda_dev, (1, 6, 6, 512, 128), (2, 1), 22)


def test_wgrad_ragged_cout(cuda_dev):
    _wgrad_case(cuda_dev, (2, 5, 11, 64, 40), (1, 2), 23)


def test_wgrad_large_grid(cuda_dev):
    _wgrad_case(cuda_dev, (8, 64, 72, 64, 128), (1, 4), 24)


def test_wgrad_taps_outside_the_map_are_exact_zeros(cuda_dev):
    """dilation (1,8) on a 7-wide map: |8| > W - 1, so the taps s = 0 and s = 2 lie outside for every pixel; autograd's gradient is exactly
    zero there and so must the kernel's be (zeros land in LDS, nothing is read)"""
    got, r = _wgrad_case(cuda_dev, ODD, (1, 8), 25)
    assert bool((r["dw"][..., 0] == 0).all()) and bool((r["dw"][..., 2] == 0).all())
    g = got.cpu()
    assert bool((g[..., 0] == 0.0).all()) and bool((g[..., 2] == 0.0).all())
    assert float(g[..., 1].abs().max()) > 1.0


def test_wgrad_accumulate(cuda_dev):
    dev = cuda_dev
    a, b = br.reference(*ODD, (1, 2), 12), br.reference(*ODD, (2, 1), 12)       # same seed: the same x, W, dy
    x, dy = a["x"].to(dev), a["dy"].to(dev)
    g = _wgrad(dev, x, dy, (1, 2), grad=torch.full((64, 64, 3, 3), 0.5, device=dev), accumulate=True)
    br.check_wgrad(g - 0.5, a["dw"], "onto 0.5")
    g = _wgrad(dev, x, dy, (1, 2), grad=torch.zeros((64, 64, 3, 3), device=dev), accumulate=True)
    g = _wgrad(dev, x, dy, (2, 1), grad=g, accumulate=True)
    br.check_wgrad(g, a["dw"] + b["dw"], "two sharers")
    g = _wgrad(dev, x, dy, (1, 2), grad=torch.full((64, 64, 3, 3), float("nan"), device=dev), accumulate=False)
    assert not bool(torch.isnan(g).any())
    br.check_wgrad(g, a["dw"], "overwrite")


def test_wgrad_channel_slices_equal_the_contiguous_call(cuda_dev):
    dev = cuda_dev
    n, h, w, cin, cout, dil = 2, 9, 7, 64, 40, (1, 2)
    r = br.reference(n, h, w, cin, cout, dil, 26)
    xbuf = torch.full((n, h, w, 128), 7.0, dtype=torch.bfloat16, device=dev)
    xbuf[..., 24:88] = r["x"].to(dev)
    dbuf = torch.full((n, h, w, 64), -3.0, dtype=torch.bfloat16, device=dev)
    dbuf[..., 16:56] = r["dy"].to(dev)
    sliced = _wgrad(dev, xbuf[..., 24:88], dbuf[..., 16:56], dil)
    dense = _wgrad(dev, r["x"].to(dev), r["dy"].to(dev), dil)
    br.check_wgrad(sliced, r["dw"], "slices")
    assert torch.equal(sliced, dense)
    assert bool((xbuf[..., :24] == 7.0).all()) and bool((xbuf[..., 88:] == 7.0).all()) and torch.equal(xbuf[..., 24:88].cpu(), r["x"])
    assert bool((dbuf[..., :16] == -3.0).all()) and bool((dbuf[..., 56:] == -3.0).all()) and torch.equal(dbuf[..., 16:56].cpu(), r["dy"])


def test_wgrad_is_bit_reproducible_and_ignores_the_workspace_contents(cuda_dev):
    dev = cuda_dev
    r = br.reference(3, 12, 12, 128, 256, (4, 1), 34)
    x, dy = r["x"].to(dev), r["dy"].to(dev)
    a = _wgrad(dev, x, dy, (4, 1), ws_fill=0.0)
    b = _wgrad(dev, x, dy, (4, 1), ws_fill=0.0)
    c = _wgrad(dev, x, dy, (4, 1), ws_fill=float("nan"))
    assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------- data gradient
def _dgrad_case(dev, shape, dil, seed):
    n, h, w, cin, cout = shape
    r = br.reference(*shape, dil, seed)
    got = _dgrad(dev, r["dy"].to(dev), r["w"], dil, cin)
    assert float(r["dx"].abs().mean()) > 0.2                       # O(1) values: the absolute floor is not what passes the test
    br.check_dgrad(got, r["dx"], br.dgrad_terms(*shape, dil, seed), "N %d %dx%d %d->%d dil %s" % (shape + (dil,)))
    return got, r


@pytest.mark.parametrize("dil", SWEEP, ids=lambda d: "d%dx%d" % d)
def test_dgrad_vs_autograd_odd_map_two_images(cuda_dev, dil):
    _dgrad_case(cuda_dev, ODD, dil, _seed(dil))


@pytest.mark.parametrize("dil", [(4, 1), (1, 2)], ids=lambda d: "d%dx%d" % d)
def test_dgrad_more_than_one_block(cuda_dev, dil):
    _dgrad_case(cuda_dev, (3, 12, 12, 128, 256), dil, 30 + _seed(dil))


def test_dgrad_channel_slices_keep_their_neighbours(cuda_dev):
    dev = cuda_dev
    n, h, w, cin, cout, dil = 2, 9, 7, 64, 64, (1, 2)       # (the forward must be served: C_in % 64 == 0)
    r = br.reference(n, h, w, cin, cout, dil, 27)
    dbuf = torch.full((n, h, w, 128), 7.0, dtype=torch.bfloat16, device=dev)
    dbuf[..., 24:88] = r["dy"].to(dev)
    xbuf = torch.full((n, h, w, 96), -3.0, dtype=torch.bfloat16, device=dev)
    _dgrad(dev, dbuf[..., 24:88], r["w"], dil, cin, dx=xbuf[..., 16:80])
    dense = _dgrad(dev, r["dy"].to(dev), r["w"], dil, cin)
    br.check_dgrad(xbuf[..., 16:80], r["dx"], br.dgrad_terms(n, h, w, cin, cout, dil, 27), "slices")
    assert torch.equal(xbuf[..., 16:80], dense)
    assert bool((xbuf[..., :16] == -3.0).all()) and bool((xbuf[..., 80:] == -3.0).all())
    assert bool((dbuf[..., :24] == 7.0).all()) and bool((dbuf[..., 88:] == 7.0).all()) and torch.equal(dbuf[..., 24:88].cpu(), r["dy"])


def test_dgrad_is_bit_reproducible_and_batch_independent(cuda_dev):
    dev = cuda_dev
    r = br.reference(*ODD, (2, 1), 28)
    dy = r["dy"].to(dev)
    a = _dgrad(dev, dy, r["w"], (2, 1), 64)
    b = _dgrad(dev, dy, r["w"], (2, 1), 64)
    assert torch.equal(a, b)
    for i in range(2):
        assert torch.equal(a[i:i + 1], _dgrad(dev, dy[i:i + 1].contiguous(), r["w"], (2, 1), 64))


def test_dgrad_undilated_equals_the_library_dgrad(cuda_dev):
    """the packed images are equal (test_packed_dgrad_image_is_the_forward_image_of_the_flipped_transposed_filter), so with dilation (1,1)
    ryolo_conv2d_dgrad on the same image is the same convolution: the same bits"""
    dev = cuda_dev
    r = br.reference(*ODD, (1, 1), 11)
    dy = r["dy"].to(dev)
    a = _dgrad(dev, dy, r["w"], (1, 1), 64)
    b = torch.empty_like(a)
    d = T.make_desc(b, 64, 3, 1, 1)
    ones, zeros = torch.ones(128, device=dev), torch.zeros(128, device=dev)
    T.conv_dgrad(d, dy, T.pack_weights_dgrad(r["w"].to(dev), 1), ones, zeros, b, False)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("cout,cin", [(64, 64), (128, 64), (256, 128), (64, 192)])
def test_packed_dgrad_image_is_the_forward_image_of_the_flipped_transposed_filter(cuda_dev, cout, cin):
    """3x3 / stride 1, both channel counts multiples of 64: ryolo_conv_pack_weights_dgrad's image == ryolo_conv_pack_weights of
    W.flip(2,3).transpose(0,1), byte for byte (size included): one packed copy serves the source layer's data gradient and every sharer's"""
    w = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(cout + cin)).to(cuda_dev)
    a = T.pack_weights_dgrad(w, 1)
    b = ops.pack_weights(w.flip(2, 3).transpose(0, 1).contiguous())
    torch.cuda.synchronize()
    assert a.numel() == b.numel() and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- refusals
def test_unsupported_arguments_return_einval_and_write_nothing(cuda_dev):
    dev = cuda_dev
    L = _lib.lib()
    n, h, w = 2, 9, 7
    x = torch.zeros((n, h, w, 64), dtype=torch.bfloat16, device=dev)
    dz = torch.zeros((n, h, w, 96), dtype=torch.bfloat16, device=dev)
    grad = torch.full((96, 64, 3, 3), 3.25, dtype=torch.float32, device=dev)
    dx = torch.full((n, h, w, 64), 3.25, dtype=torch.bfloat16, device=dev)
    ws = torch.full((1 << 20,), 3.25, dtype=torch.float32, device=dev)
    packed = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    ones, zeros = torch.ones(128, device=dev), torch.zeros(128, device=dev)
    s = _lib.stream_ptr(dev)

    def wg(d, dil, xp=x.data_ptr(), dzp=dz.data_ptr(), gp=grad.data_ptr(), wsp=ws.data_ptr(), wsb=ws.numel() * 4, dz_cs=None):
        return L.ryolo_conv2d_dilated_wgrad(C.byref(d), dil[0], dil[1], xp, dzp, d.Cout if dz_cs is None else dz_cs, gp, 0, wsp, wsb, s)

    def dg(d, dil, dzp=dz.data_ptr(), pk=packed.data_ptr(), dxp=dx.data_ptr()):
        return L.ryolo_conv2d_dilated_dgrad(C.byref(d), dil[0], dil[1], dzp, d.Cout, pk, ones.data_ptr(), zeros.data_ptr(), dxp, s)

    good = T.dilated_desc(n, h, w, 64, 64)
    assert T.conv_dilated_wgrad_ws_bytes(good, (1, 2)) <= ws.numel() * 4
    assert wg(T.dilated_desc(n, h, w, 32, 64), (1, 2)) == EINVAL                        # C_in 32
    assert dg(T.dilated_desc(n, h, w, 32, 64), (1, 2)) == EINVAL
    assert dg(T.dilated_desc(n, h, w, 64, 96), (1, 2)) == EINVAL                        # C_out 96: the data gradient's K channels
    for dil in ((0, 1), (1, 0), (33, 1), (1, 33)):
        assert wg(good, dil) == EINVAL and dg(good, dil) == EINVAL
    assert wg(good, (1, 2), wsb=T.conv_dilated_wgrad_ws_bytes(good, (1, 2)) - 4) == EINVAL      # a short workspace
    for null in ("xp", "dzp", "gp", "wsp"):
        assert wg(good, (1, 2), **{null: None}) == EINVAL
    for null in ("dzp", "pk", "dxp"):
        assert dg(good, (1, 2), **{null: None}) == EINVAL
    assert wg(good, (1, 2), dz_cs=60) == EINVAL                                         # a pixel stride below the channel count
    torch.cuda.synchronize()
    assert bool((grad == 3.25).all()) and bool((dx == 3.25).all()) and bool((ws == 3.25).all())
    # ... and the same descriptor with nothing wrong is served (the refusals above are not an accident of the harness)
    assert wg(good, (1, 2)) == 0
    torch.cuda.synchronize()
    assert bool((grad[:64] == 0).all()) and bool((grad[64:] == 3.25).all())


# ---------------------------------------------------------------------------------------------------- the autograd Function
def test_shared_dilated_conv_function(cuda_dev, monkeypatch):
    dev = cuda_dev
    dil = (1, 2)
    r = br.reference(*ODD, dil, 12)
    x = r["x"].float().permute(0, 3, 1, 2).contiguous().to(dev).requires_grad_(True)      # NCHW fp32 holding bf16 values
    wt = r["w"].to(dev).requires_grad_(True)
    dy = r["dy"].float().permute(0, 3, 1, 2).contiguous().to(dev)
    y = T.SharedDilatedConv.apply(x, wt, dil)
    assert y.shape == (2, 64, 9, 7) and y.dtype == torch.float32
    saved = [t for t in y.grad_fn.saved_tensors if t.dim() == 4 and t.shape[-1] == 64 and t.dtype == torch.bfloat16]
    assert len(saved) == 1 and tuple(saved[0].shape) == (2, 9, 7, 64)               # the bf16 NHWC x is what is kept, not the fp32 input
    assert not any(tuple(t.shape) == (2, 64, 9, 7) for t in y.grad_fn.saved_tensors)
    (y * dy).sum().backward()
    torch.cuda.synchronize()
    y_nhwc = y.detach().permute(0, 2, 3, 1).cpu()
    err = (y_nhwc - r["y"].to(torch.bfloat16).float()).abs()
    assert bool((err <= br.DGRAD_REL * r["y"].abs() + br.DGRAD_ABS).all()), err.max().item()
    br.check_dgrad(x.grad.permute(0, 2, 3, 1), r["dx"], br.dgrad_terms(*ODD, dil, 12), "Function")
    br.check_wgrad(wt.grad, r["dw"], "Function")

    # an input that needs no gradient: no data-gradient launch, None returned for it
    calls = []
    real = T.conv_dilated_dgrad
    monkeypatch.setattr(T, "conv_dilated_dgrad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x2 = x.detach()
    w2 = r["w"].to(dev).requires_grad_(True)
    y2 = T.SharedDilatedConv.apply(x2, w2, dil)
    fn = y2.grad_fn
    (y2 * dy).sum().backward()
    torch.cuda.synchronize()
    assert calls == [] and x2.grad is None and fn.next_functions[0][0] is None
    assert torch.equal(w2.grad, wt.grad)
    assert torch.equal(y2, y)
