"""Python-side handles on the C ABI's convolution block and layout converters (include/ryolo.h).

Plumbing only: torch supplies device memory and the current stream; all arithmetic happens in
csrc/conv.hip.  Tensors here are NHWC bf16 `torch.Tensor`s of shape [N, H, W, C] whose last-dim stride is 1
and whose pixel stride (stride(2)) may exceed C (a channel slice of a wider concat buffer).
"""
import ctypes as C

import torch

from .. import _lib
from .._lib import ACT_LEAKY, ACT_LINEAR, ACT_MISH, ConvDesc  # noqa: F401  (part of this module's interface)


def cpad(c, m=128):
    return (c + m - 1) // m * m


def pack_weights(weight, cin_pad=None, out=None):
    """weight: fp32 [Cout, Cin, k, k] on the GPU (nn.Conv2d.weight layout) -> packed bf16 image (uint8 tensor)."""
    assert weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4
    cout, cin, k, k2 = weight.shape
    assert k == k2
    cin_pad = cin_pad or (cin + 7) // 8 * 8
    L = _lib.lib()
    nbytes = L.ryolo_conv_packed_weight_bytes(cout, cin_pad, k)
    if nbytes == 0:
        raise RuntimeError("unsupported conv weight shape %s" % (tuple(weight.shape),))
    w = weight.contiguous()
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    with torch.cuda.device(weight.device):
        _lib.check(L.ryolo_conv_pack_weights(w.data_ptr(), cout, cin, k, cin_pad, out.data_ptr(),
                                             _lib.stream_ptr(weight.device)), "ryolo_conv_pack_weights")
    return out


def pad_vec(v, n, fill=0.0):
    out = torch.full((n,), fill, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v.float()
    return out


def _check_nhwc(t, name):
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4 and t.stride(3) == 1):
        raise RuntimeError("%s must be an NHWC bf16 GPU tensor with unit channel stride" % name)
    n, h, w, c = t.shape
    cs = t.stride(2)
    if t.stride(1) != w * cs or t.stride(0) != h * w * cs:
        raise RuntimeError("%s: pixels must be densely packed rows of `pixel stride` elements" % name)
    return cs


def conv2d_bn_act(x, packed_w, scale, shift, cout, ksize, stride=1, pad=None, act=ACT_LINEAR, slope=0.1,
                  residual=None, out=None, upsample=1, tile=0):
    """y = upsample(act(conv(x, W) * scale + shift) + residual); x, residual, out: NHWC bf16 (possibly slices)."""
    in_cs = _check_nhwc(x, "x")
    n, h, w, cin = x.shape
    pad = (ksize - 1) // 2 if pad is None else pad
    ho = (h + 2 * pad - ksize) // stride + 1
    wo = (w + 2 * pad - ksize) // stride + 1
    if out is None:
        out = torch.empty((n, ho * upsample, wo * upsample, cout), dtype=torch.bfloat16, device=x.device)
    out_cs = _check_nhwc(out, "out")
    assert tuple(out.shape) == (n, ho * upsample, wo * upsample, cout), (tuple(out.shape), (n, ho, wo, cout))
    res_cs = 0
    if residual is not None:
        res_cs = _check_nhwc(residual, "residual")
        assert tuple(residual.shape) == (n, ho, wo, cout)
    d = ConvDesc(n, h, w, cin, cout, ksize, stride, pad, in_cs, out_cs, res_cs, act, float(slope), upsample, tile)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ryolo_conv2d_bn_act(C.byref(d), x.data_ptr(), packed_w.data_ptr(), scale.data_ptr(),
                                            shift.data_ptr(), residual.data_ptr() if residual is not None else None,
                                            out.data_ptr(), _lib.stream_ptr(x.device))
    _lib.check(rc, "ryolo_conv2d_bn_act")
    return out


def conv2d_dilated_supported(d, dil):
    """does csrc/conv_dil.hip serve the dilated 3x3 conv of descriptor d (no device call)"""
    dh, dw = (dil, dil) if isinstance(dil, int) else dil
    return bool(_lib.lib().ryolo_conv2d_dilated_supported(C.byref(d), int(dh), int(dw)))


def conv2d_dilated(x, packed_w, scale, shift, cout, dil, act=ACT_LINEAR, slope=0.1, residual=None, out=None):
    """y = act(conv3x3(x, W, padding=dil, dilation=dil) * scale + shift) + residual (csrc/conv_dil.hip); dil = (dh, dw); packed_w is the
    image pack_weights makes for the undilated 3x3 layer; x, residual, out: NHWC bf16 (possibly slices), the output is H x W."""
    in_cs = _check_nhwc(x, "x")
    n, h, w, cin = x.shape
    dh, dw = (dil, dil) if isinstance(dil, int) else dil
    if out is None:
        out = torch.empty((n, h, w, cout), dtype=torch.bfloat16, device=x.device)
    out_cs = _check_nhwc(out, "out")
    assert tuple(out.shape) == (n, h, w, cout), (tuple(out.shape), (n, h, w, cout))
    res_cs = 0
    if residual is not None:
        res_cs = _check_nhwc(residual, "residual")
        assert tuple(residual.shape) == (n, h, w, cout)
    d = ConvDesc(n, h, w, cin, cout, 3, 1, 1, in_cs, out_cs, res_cs, act, float(slope), 1, 0)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ryolo_conv2d_dilated(C.byref(d), int(dh), int(dw), x.data_ptr(), packed_w.data_ptr(), scale.data_ptr(),
                                             shift.data_ptr(), residual.data_ptr() if residual is not None else None,
                                             out.data_ptr(), _lib.stream_ptr(x.device))
    _lib.check(rc, "ryolo_conv2d_dilated")
    return out


def se_workspace(n, h, w, c, device):
    """scratch of one ryolo_se_nhwc call (partial pixel sums + gates)"""
    nbytes = _lib.lib().ryolo_se_workspace_bytes(n, h, w, c)
    if nbytes == 0:
        raise RuntimeError("se: unsupported shape N %d, H %d, W %d, C %d (C must be a multiple of 8 from 16 to 2048)" % (n, h, w, c))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def se_nhwc(x, w1, w2, out=None, gate_out=None, workspace=None):
    """y = x * sigmoid(W2 . relu(W1 . mean_hw(x))) -- SELayer.forward on NHWC bf16 (possibly slices); w1 [hidden, C] and w2 [C, hidden]
    fp32 contiguous (fc.0.weight / fc.2.weight); gate_out: fp32 [N, C] that receives the gates."""
    x_cs = _check_nhwc(x, "x")
    n, h, w, c = x.shape
    hidden = w1.shape[0]
    for t, shape, name in ((w1, (hidden, c), "w1"), (w2, (c, hidden), "w2")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError("%s must be a contiguous fp32 GPU tensor of shape %s" % (name, shape))
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.bfloat16, device=x.device)
    y_cs = _check_nhwc(out, "out")
    assert tuple(out.shape) == (n, h, w, c), (tuple(out.shape), (n, h, w, c))
    if gate_out is not None:
        assert gate_out.is_cuda and gate_out.dtype == torch.float32 and gate_out.is_contiguous() and tuple(gate_out.shape) == (n, c)
    if workspace is None:
        workspace = se_workspace(n, h, w, c, x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ryolo_se_nhwc(x.data_ptr(), x_cs, w1.data_ptr(), w2.data_ptr(), hidden, out.data_ptr(), y_cs, n, h, w, c,
                                      gate_out.data_ptr() if gate_out is not None else None, workspace.data_ptr(), workspace.numel(),
                                      _lib.stream_ptr(x.device))
    _lib.check(rc, "ryolo_se_nhwc")
    return out


def pair_descs(x, first, second, out_cs=None):
    """ConvDesc pair for conv2d_bn_act_pair; first / second = dicts(cout, ksize, stride, pad, act, slope)"""
    in_cs = _check_nhwc(x, "x")
    n, h, w, cin = x.shape
    a = ConvDesc(n, h, w, cin, first['cout'], first['ksize'], first['stride'], first['pad'], in_cs, first['cout'], 0, first['act'],
                 float(first['slope']), 1, 0)
    h1 = (h + 2 * first['pad'] - first['ksize']) // first['stride'] + 1
    w1 = (w + 2 * first['pad'] - first['ksize']) // first['stride'] + 1
    b = ConvDesc(n, h1, w1, first['cout'], second['cout'], second['ksize'], second['stride'], second['pad'], first['cout'],
                 out_cs or second['cout'], 0, second['act'], float(second['slope']), 1, 0)
    return a, b


def conv_pair_supported(x, first, second, shortcut_from_input):
    a, b = pair_descs(x, first, second)
    return bool(_lib.lib().ryolo_conv_pair_supported(C.byref(a), C.byref(b), 1 if shortcut_from_input else 0))


def conv2d_bn_act_pair(x, first, second, packed1, scale1, shift1, packed2, scale2, shift2, shortcut_from_input=False, out=None):
    """y = block2(block1(x)) [+ x]: two conv blocks in one launch, the tensor between them never stored (csrc/conv_stem.hip)."""
    n, h, w, cin = x.shape
    h1 = (h + 2 * first['pad'] - first['ksize']) // first['stride'] + 1
    w1 = (w + 2 * first['pad'] - first['ksize']) // first['stride'] + 1
    h2 = (h1 + 2 * second['pad'] - second['ksize']) // second['stride'] + 1
    w2 = (w1 + 2 * second['pad'] - second['ksize']) // second['stride'] + 1
    if out is None:
        out = torch.empty((n, h2, w2, second['cout']), dtype=torch.bfloat16, device=x.device)
    out_cs = _check_nhwc(out, "out")
    assert tuple(out.shape) == (n, h2, w2, second['cout'])
    a, b = pair_descs(x, first, second, out_cs)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ryolo_conv2d_bn_act_pair(C.byref(a), C.byref(b), x.data_ptr(), packed1.data_ptr(), scale1.data_ptr(), shift1.data_ptr(),
                                                 packed2.data_ptr(), scale2.data_ptr(), shift2.data_ptr(), 1 if shortcut_from_input else 0,
                                                 out.data_ptr(), _lib.stream_ptr(x.device))
    _lib.check(rc, "ryolo_conv2d_bn_act_pair")
    return out


_IGEMM_TILES = {1: '128x128', 2: '256x64', 3: '256x32', 4: '256x128', 6: '128x128(4x2)', 7: '128x128(2x2)'}


def conv_kernel_name(n, h, w, cin, cout, ksize, stride=1, pad=None, in_cs=None, out_cs=None, res_cs=0, upsample=1, tile=0,
                     residual=False, statistics=False):
    """Name of the kernel the library's dispatch picks for this conv on the current device (the launch's plan, nothing is launched):
    what the per-kernel tables of bench.py and the profiles call it."""
    pad = (ksize - 1) // 2 if pad is None else pad
    d = ConvDesc(n, h, w, cin, cout, ksize, stride, pad, in_cs or cin, out_cs or cout, res_cs or (cout if residual else 0), 1, 0.1,
                 upsample, tile)
    code = _lib.lib().ryolo_conv_kernel_choice(C.byref(d), 1 if residual else 0, 1 if statistics else 0)
    return kernel_name_of(code, ksize, stride, cin)


def kernel_name_of(code, ksize, stride, cin):
    """the name bench.py / the profiles use for a RYOLO_CONV_KERNEL_* code (include/ryolo.h)"""
    if code in (1, 2):
        return 'conv_mp<k%d,%dx256>' % (ksize, 256 if code == 1 else 192)
    if code == 3:
        return 'conv_mq<k%d,128x256>' % ksize
    if code == 4:
        return 'conv3x3_c8_direct'
    if code == 5:
        return 'conv3x3_c32_halo<s%d>' % stride
    if code == 6:
        return 'conv_pw<k1,K%d>' % cin
    if code == 7:
        return 'conv_stem_dgrad'
    if code == 8:
        return 'conv0_halo<c8>'
    if code == 11:
        return 'conv3x3_c64_halo'
    if code in (9, 10):
        return 'conv_mq<k%d,%dx128>' % (ksize, 128 if code == 9 else 64)
    if code >= 16:
        return 'conv_igemm<k%d,%s>' % (ksize, _IGEMM_TILES.get(code - 16, 'tile%d' % (code - 16)))
    return 'conv<?>'


def nchw_f32_to_nhwc_bf16(x, cpad_to=8):
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    n, c, h, w = x.shape
    cp = (c + cpad_to - 1) // cpad_to * cpad_to
    y = torch.empty((n, h, w, cp), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().ryolo_nchw_f32_to_nhwc_bf16(x.data_ptr(), n, c, h, w, cp, y.data_ptr(),
                                                          _lib.stream_ptr(x.device)), "ryolo_nchw_f32_to_nhwc_bf16")
    return y


def letterbox_augment(cache, src_index, params, seed, H, W, out=None):
    """One launch of csrc/augment.hip: batch slot n = the cached image src_index[n], sampled through the matrix of params[n] and put
    through its photometric stages (include/ryolo.h: ryolo_letterbox_augment) -> NHWC8Batch of [N, H, W, 8].
    cache: the device image cache (utils.datasets.DeviceImageCache: .pixels uint8, .img_offset int64 [n], .img_hw int32 [n, 2]);
    src_index: int32 [N]; params: fp32 [N, 16]; both on the cache's device.  out: a bf16 [N, H, W, 8] tensor to write into."""
    from .nhwc_batch import NHWC8Batch
    L = _lib.lib()
    pixels, offs, hw = cache.pixels, cache.img_offset, cache.img_hw
    dev = pixels.device
    if not (pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.is_contiguous()):
        raise RuntimeError("cache.pixels must be a contiguous uint8 GPU tensor")
    n_cache = offs.numel()
    if not (offs.dtype == torch.int64 and offs.is_contiguous() and offs.device == dev and hw.dtype == torch.int32 and hw.is_contiguous()
            and hw.device == dev and tuple(hw.shape) == (n_cache, 2)):
        raise RuntimeError("cache.img_offset / cache.img_hw must be int64 [n] / int32 [n, 2] tensors on the cache's device")
    if not torch.is_tensor(src_index):
        src_index = torch.tensor(list(src_index), dtype=torch.int32, device=dev)
    if not torch.is_tensor(params):
        params = torch.as_tensor(params, dtype=torch.float32).to(dev)
    n = src_index.numel()
    if not (src_index.dtype == torch.int32 and src_index.dim() == 1 and src_index.is_contiguous() and src_index.device == dev):
        raise RuntimeError("src_index must be a contiguous int32 [N] tensor on the cache's device")
    if not (params.dtype == torch.float32 and params.is_contiguous() and params.device == dev
            and tuple(params.shape) == (n, L.ryolo_aug_nparam())):
        raise RuntimeError("params must be a contiguous fp32 [N, %d] tensor on the cache's device" % L.ryolo_aug_nparam())
    if out is None:
        out = torch.empty((n, H, W, 8), dtype=torch.bfloat16, device=dev)
    elif not (out.dtype == torch.bfloat16 and out.is_contiguous() and out.device == dev and tuple(out.shape) == (n, H, W, 8)):
        raise RuntimeError("out must be a contiguous bf16 [N, H, W, 8] tensor on the cache's device")
    with torch.cuda.device(dev):
        _lib.check(L.ryolo_letterbox_augment(pixels.data_ptr(), offs.data_ptr(), hw.data_ptr(), n_cache, src_index.data_ptr(),
                                             params.data_ptr(), int(seed), n, int(H), int(W), out.data_ptr(), _lib.stream_ptr(dev)),
                   "ryolo_letterbox_augment")
    return NHWC8Batch(out)


def letterbox_area(cache, src_index, place, H, W, out=None):
    """ceil(N / 64) launches of csrc/letterbox_area.hip: batch slot n = the cached image src_index[n] resized to place[n][2:] (area
    averaging when that is smaller, bilinear otherwise) with its top left corner at place[n][:2], 128 around it (include/ryolo.h:
    ryolo_letterbox_area) -> NHWC8Batch of [N, H, W, 8].
    cache: as for letterbox_augment; src_index: int32 [N] on the cache's device; place: [N, 4] integer rows (left, top, new_w, new_h) on the
    HOST (a numpy array, a list, a CPU tensor: utils.datasets.place_rows); out: a bf16 [N, H, W, 8] tensor to write into."""
    import numpy as np
    from .nhwc_batch import NHWC8Batch
    L = _lib.lib()
    pixels, offs, hw = cache.pixels, cache.img_offset, cache.img_hw
    dev = pixels.device
    if not (pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.is_contiguous()):
        raise RuntimeError("cache.pixels must be a contiguous uint8 GPU tensor")
    n_cache = offs.numel()
    if not (offs.dtype == torch.int64 and offs.is_contiguous() and offs.device == dev and hw.dtype == torch.int32 and hw.is_contiguous()
            and hw.device == dev and tuple(hw.shape) == (n_cache, 2)):
        raise RuntimeError("cache.img_offset / cache.img_hw must be int64 [n] / int32 [n, 2] tensors on the cache's device")
    if not torch.is_tensor(src_index):
        src_index = torch.tensor(list(src_index), dtype=torch.int32, device=dev)
    n = src_index.numel()
    if not (src_index.dtype == torch.int32 and src_index.dim() == 1 and src_index.is_contiguous() and src_index.device == dev):
        raise RuntimeError("src_index must be a contiguous int32 [N] tensor on the cache's device")
    if torch.is_tensor(place):
        if place.is_cuda or place.is_floating_point():
            raise RuntimeError("place must be integer [N, 4] rows in host memory, not a %s tensor on %s" % (place.dtype, place.device))
        place = place.numpy()
    place = np.asarray(place)
    if not (place.dtype.kind in 'iu' and place.shape == (n, 4)):
        raise RuntimeError("place must be integer [N, 4] rows (left, top, new_w, new_h), not %s %s" % (place.dtype, place.shape))
    place = np.ascontiguousarray(place, dtype=np.int32)
    if out is None:
        out = torch.empty((n, H, W, 8), dtype=torch.bfloat16, device=dev)
    elif not (out.dtype == torch.bfloat16 and out.is_contiguous() and out.device == dev and tuple(out.shape) == (n, H, W, 8)):
        raise RuntimeError("out must be a contiguous bf16 [N, H, W, 8] tensor on the cache's device")
    with torch.cuda.device(dev):
        _lib.check(L.ryolo_letterbox_area(pixels.data_ptr(), offs.data_ptr(), hw.data_ptr(), n_cache, src_index.data_ptr(),
                                          place.ctypes.data, n, int(H), int(W), out.data_ptr(), _lib.stream_ptr(dev)),
                   "ryolo_letterbox_area")
    return NHWC8Batch(out)


def _check_det(det):
    if not (torch.is_tensor(det) and det.is_cuda and det.dtype == torch.float32 and det.dim() == 2 and det.shape[1] == 8
            and det.is_contiguous()):
        raise RuntimeError("det must be a contiguous fp32 [M, 8] GPU tensor")


def det_rescale(det, det_off, geom):
    """scale_coords(...).round() of the reference in place on the flat detection rows of a batch (include/ryolo.h: ryolo_det_rescale).
    det: fp32 [M, 8]; det_off: int32 [bs + 1] row offsets per image; geom: fp32 [bs, 3] rows (gain, pad_x, pad_y)
    (utils.detect_images.rescale_geometry), all on one GPU.  Returns det."""
    _check_det(det)
    dev = det.device
    if not (torch.is_tensor(det_off) and det_off.dtype == torch.int32 and det_off.dim() == 1 and det_off.numel() >= 2
            and det_off.is_contiguous() and det_off.device == dev):
        raise RuntimeError("det_off must be a contiguous int32 [bs + 1] tensor on det's device")
    bs = det_off.numel() - 1
    if not (torch.is_tensor(geom) and geom.dtype == torch.float32 and geom.is_contiguous() and geom.device == dev
            and tuple(geom.shape) == (bs, 3)):
        raise RuntimeError("geom must be a contiguous fp32 [bs, 3] tensor on det's device")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ryolo_det_rescale(det.data_ptr(), det.shape[0], det_off.data_ptr(), bs, geom.data_ptr(),
                                                _lib.stream_ptr(dev)), "ryolo_det_rescale")
    return det


def det_quads(det, out=None):
    """xywha2icdar of the reference for every row of det (fp32 [M, 8]) -> int32 [M, 8] rows (x, y of tl, tr, br, bl)
    (include/ryolo.h: ryolo_det_quads)."""
    _check_det(det)
    dev = det.device
    if out is None:
        out = torch.empty((det.shape[0], 8), dtype=torch.int32, device=dev)
    elif not (out.dtype == torch.int32 and out.is_contiguous() and out.device == dev and tuple(out.shape) == (det.shape[0], 8)):
        raise RuntimeError("out must be a contiguous int32 [M, 8] tensor on det's device")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ryolo_det_quads(det.data_ptr(), det.shape[0], out.data_ptr(), _lib.stream_ptr(dev)), "ryolo_det_quads")
    return out


def det_corners(det, out=None):
    """get_rotated_coors of the reference for every row of det (fp32 [M, 8]) -> int32 [M, 8] rows (x, y of the corners (xmin, ymin),
    (xmin, ymax), (xmax, ymax), (xmax, ymin) after the turn, in that order): the outlines draw_quads draws
    (include/ryolo.h: ryolo_det_corners)."""
    _check_det(det)
    dev = det.device
    if out is None:
        out = torch.empty((det.shape[0], 8), dtype=torch.int32, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.int32 and out.is_contiguous() and out.device == dev
              and tuple(out.shape) == (det.shape[0], 8)):
        raise RuntimeError("out must be a contiguous int32 [M, 8] tensor on det's device")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ryolo_det_corners(det.data_ptr(), det.shape[0], out.data_ptr(), _lib.stream_ptr(dev)), "ryolo_det_corners")
    return out


DRAW_ROWS_PER_PASS = 256      # rows a workgroup of csrc/draw.hip culls per pass (ryolo_draw_rows_per_pass(); a CPU test holds the two equal)
DRAW_MAX_SIDE = 16384         # the largest image side ryolo_draw_quads accepts


def draw_quads(cache_or_pixels, quad, det_off, color, thick, labels=None, out=None):
    """One launch of csrc/draw.hip: the outlines quad[r] (int32 [M, 8], det_corners) and the label bitmaps painted over the pixels of an
    image cache, the highest row on top (include/ryolo.h: ryolo_draw_quads).  Returns the drawn pixels, a uint8 tensor laid out like
    cache.pixels; the cache itself is not written unless out is cache.pixels.
    cache_or_pixels: a DeviceImageCache, or the tuple (pixels, img_offset, img_hw, hw) of its fields (hw: the HOST list of (h, w));
    det_off: int32 [n_img + 1] row offsets per image; color: uint8 [M, 4] RGBx; thick: one int 1..255 or one per image, on the HOST;
    labels: None or (lab_bits uint8 [nbytes], lab_off int64 [M], lab_rect int32 [M, 4] rows (x, y, w, h)) (utils.plots.pack_labels);
    quad, det_off, color and labels on the pixels' device.  out: a uint8 tensor like pixels to draw into (pixels itself: in place)."""
    import numpy as np
    if isinstance(cache_or_pixels, (tuple, list)):
        if len(cache_or_pixels) != 4:
            raise RuntimeError("cache_or_pixels must be a DeviceImageCache or the tuple (pixels, img_offset, img_hw, hw)")
        pixels, offs, hw, host_hw = cache_or_pixels
    else:
        pixels, offs, hw, host_hw = cache_or_pixels.pixels, cache_or_pixels.img_offset, cache_or_pixels.img_hw, cache_or_pixels.hw
    if not (torch.is_tensor(pixels) and pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.is_contiguous()):
        raise RuntimeError("cache.pixels must be a contiguous uint8 [nbytes] GPU tensor")
    dev = pixels.device
    n_img = offs.numel() if torch.is_tensor(offs) else -1
    if not (n_img >= 1 and offs.dtype == torch.int64 and offs.is_contiguous() and offs.device == dev and torch.is_tensor(hw)
            and hw.dtype == torch.int32 and hw.is_contiguous() and hw.device == dev and tuple(hw.shape) == (n_img, 2)):
        raise RuntimeError("cache.img_offset / cache.img_hw must be int64 [n] / int32 [n, 2] tensors on the cache's device")
    host_hw = [(int(h), int(w)) for h, w in host_hw]
    if len(host_hw) != n_img or min(min(s) for s in host_hw) < 1 or max(max(s) for s in host_hw) > DRAW_MAX_SIDE:
        raise RuntimeError("cache.hw must hold the %d (h, w) of the images, every side in 1..%d" % (n_img, DRAW_MAX_SIDE))
    if n_img > _lib.lib().ryolo_draw_max_images():
        raise RuntimeError("cache holds %d images: draw_quads takes at most %d per call" % (n_img, _lib.lib().ryolo_draw_max_images()))
    if not (torch.is_tensor(quad) and quad.dtype == torch.int32 and quad.dim() == 2 and quad.shape[1] == 8 and quad.is_contiguous()
            and quad.device == dev):
        raise RuntimeError("quad must be a contiguous int32 [M, 8] tensor on the pixels' device")
    m = quad.shape[0]
    if not (torch.is_tensor(det_off) and det_off.dtype == torch.int32 and det_off.dim() == 1 and det_off.numel() == n_img + 1
            and det_off.is_contiguous() and det_off.device == dev):
        raise RuntimeError("det_off must be a contiguous int32 [n_img + 1] tensor on the pixels' device (n_img = %d)" % n_img)
    if not (torch.is_tensor(color) and color.dtype == torch.uint8 and color.is_contiguous() and color.device == dev
            and tuple(color.shape) == (m, 4)):
        raise RuntimeError("color must be a contiguous uint8 [M, 4] (RGBx) tensor on the pixels' device")
    if torch.is_tensor(thick):
        if thick.is_cuda or thick.is_floating_point():
            raise RuntimeError("thick must be integers in host memory, not a %s tensor on %s" % (thick.dtype, thick.device))
        thick = thick.numpy()
    thick = np.asarray(thick)
    if thick.ndim == 0:
        thick = np.full(n_img, thick)
    if not (thick.dtype.kind in 'iu' and thick.shape == (n_img,) and thick.min() >= 1 and thick.max() <= 255):
        raise RuntimeError("thick must be one integer in 1..255 or one per image (%d), not %s %s" % (n_img, thick.dtype, thick.shape))
    thick = np.ascontiguousarray(thick, dtype=np.int32)
    bits_ptr = off_ptr = rect_ptr = None
    if labels is not None:
        if not (isinstance(labels, (tuple, list)) and len(labels) == 3 and all(torch.is_tensor(t) for t in labels)):
            raise RuntimeError("labels must be None or the tuple (lab_bits, lab_off, lab_rect) of tensors")
        bits, loff, rect = labels
        if not (bits.dtype == torch.uint8 and bits.dim() == 1 and bits.is_contiguous() and bits.device == dev):
            raise RuntimeError("labels: lab_bits must be a contiguous uint8 [nbytes] tensor on the pixels' device")
        if not (loff.dtype == torch.int64 and loff.is_contiguous() and loff.device == dev and tuple(loff.shape) == (m,)):
            raise RuntimeError("labels: lab_off must be a contiguous int64 [M] tensor on the pixels' device")
        if not (rect.dtype == torch.int32 and rect.is_contiguous() and rect.device == dev and tuple(rect.shape) == (m, 4)):
            raise RuntimeError("labels: lab_rect must be a contiguous int32 [M, 4] tensor on the pixels' device")
        # every rectangle must lie inside lab_bits (lab_off[r] + lw * lh <= nbytes: the caller's duty, pack_labels keeps it), so
        # without a single label byte every lw * lh is 0 and the call is the one without labels
        if m and bits.numel():
            bits_ptr, off_ptr, rect_ptr = bits.data_ptr(), loff.data_ptr(), rect.data_ptr()
    if out is None:
        out = torch.empty_like(pixels)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev
              and tuple(out.shape) == tuple(pixels.shape)):
        raise RuntimeError("out must be a contiguous uint8 tensor of the shape of the pixels, on their device")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ryolo_draw_quads(pixels.data_ptr(), out.data_ptr(), offs.data_ptr(), hw.data_ptr(), n_img,
                                               max(h for h, _ in host_hw), max(w for _, w in host_hw), quad.data_ptr() if m else None,
                                               det_off.data_ptr(), m, color.data_ptr() if m else None, thick.ctypes.data, bits_ptr, off_ptr,
                                               rect_ptr, _lib.stream_ptr(dev)), "ryolo_draw_quads")
    return out


def nhwc_bf16_to_nchw_f32(x):
    cs = _check_nhwc(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().ryolo_nhwc_bf16_to_nchw_f32(x.data_ptr(), n, c, h, w, cs, y.data_ptr(),
                                                          _lib.stream_ptr(x.device)), "ryolo_nhwc_bf16_to_nchw_f32")
    return y
