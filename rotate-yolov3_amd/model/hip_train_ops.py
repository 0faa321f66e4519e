"""Python handles on the training-step entry points of the C ABI (include/ryolo.h; csrc/train.hip, csrc/wgrad.hip, csrc/conv_dgrad.hip + csrc/conv.hip;
csrc/conv_dil.hip + csrc/wgrad_dil.hip for the dilated shared convs of the matrix cfgs; csrc/se_bwd.hip for the se blocks).
Plumbing only: torch owns the device memory and the stream."""
import ctypes as C

import torch

from .. import _lib
from .._lib import PackJob, WgradReduceJob
from . import hip_ops
from .hip_ops import ConvDesc, _check_nhwc, cpad, pack_weights

ARC_FOCAL, ARC_UBCE, ARC_UCE = 1, 2, 4


def arc_flags(arc):
    """compute_loss's arc string (model/loss.py:268: default, uCE, uBCE, each optionally with an F for the focal wrappers) ->
    the flag word of ryolo_yolo_loss_arc"""
    f = ARC_FOCAL if 'F' in arc else 0
    if 'default' in arc:
        return f
    if 'BCE' in arc:
        return f | ARC_UBCE
    if 'CE' in arc:
        return f | ARC_UCE
    raise ValueError("unknown arc %r" % (arc,))


class _JobTable(object):
    """Jobs of one batched launch: ctypes records of type `job` whose fill function left the job's block count in block_end.  finalize()
    turns the counts into each job's range of the launch's blocks and uploads the table (from the host: outside any stream capture),
    run() is the ONE launch of the entry point `entry`(table, n, total_blocks, stream)."""
    job = entry = None

    def __init__(self, device):
        self.device = device
        self.jobs = []
        self.keep = []

    def finalize(self):
        arr = (self.job * len(self.jobs))()
        blk = 0
        for q, j in enumerate(self.jobs):
            nb = j.block_end
            j.block_begin, j.block_end = blk, blk + nb
            blk += nb
            arr[q] = j
        self.total_blocks = blk
        self.dev_jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.n = len(self.jobs)

    def run(self):
        _lib.check(getattr(_lib.lib(), self.entry)(self.dev_jobs.data_ptr(), self.n, self.total_blocks, _s(self.device)), self.entry)


class WgradReduceBatch(_JobTable):
    """The split-K reduces of several layers as one launch (csrc/wgrad.hip: wgrad_reduce_batch_kernel).  Every layer keeps its partial
    tiles in its OWN workspace (conv_wgrad_partials); add() describes a layer's reduce, finalize() uploads the job table, run() reduces all
    of them -- bit-identical to the per-layer reduces."""
    job, entry = WgradReduceJob, "ryolo_conv_wgrad_reduce_batch"

    def add(self, d, cin_real, ws, grad, accumulate):
        j = WgradReduceJob()
        n = _lib.lib().ryolo_conv_wgrad_reduce_job_fill(C.byref(j), C.byref(d), cin_real, ws.data_ptr(), grad.data_ptr(), 1 if accumulate else 0)
        if n <= 0:
            raise RuntimeError("ryolo_conv_wgrad_reduce_job_fill failed")
        self.jobs.append(j)
        self.keep.append((ws, grad))


class WeightPackBatch(_JobTable):
    """Every weight pack of a training step (forward layout + dgrad classes of each conv) as one launch."""
    job, entry = PackJob, "ryolo_conv_pack_batch"

    def add(self, weight, stride, cin_pad, packed_fwd, packed_dgrad):
        cout, cin, k, _ = weight.shape
        tmp = (PackJob * 8)()      # forward + up to 4 classic + 2 x-fused dgrad images
        n = _lib.lib().ryolo_conv_pack_job_fill(tmp, weight.data_ptr(), cout, cin, k, stride, cin_pad, packed_fwd.data_ptr(),
                                                packed_dgrad.data_ptr() if packed_dgrad is not None else None)
        if n <= 0:
            raise RuntimeError("ryolo_conv_pack_job_fill failed")
        for q in range(n):
            j = PackJob()
            C.memmove(C.byref(j), C.byref(tmp[q]), C.sizeof(PackJob))
            self.jobs.append(j)


def _s(dev):
    return _lib.stream_ptr(dev)


def make_desc(x, cout, ksize, stride, pad, out_cs=None, tile=0):
    in_cs = _check_nhwc(x, "x")
    n, h, w, cin = x.shape
    return ConvDesc(n, h, w, cin, cout, ksize, stride, pad, in_cs, out_cs or cout, 0, 0, 0.0, 1, tile)


def stat_rows():
    """Partial rows of the statistics scratch the conv kernels spread their atomics over (a library constant)."""
    d = ConvDesc(1, 8, 8, 8, 8, 1, 1, 0, 8, 8, 0, 0, 0.0, 1, 0)
    rows = _lib.lib().ryolo_conv_stat_rows(C.byref(d))
    if rows <= 0:
        raise RuntimeError("ryolo_conv_stat_rows failed")
    return rows


def conv_fwd_stats(d, x, packed_w, ones, shift, z, part=None, clear=True):
    """z = conv(x, W) (linear; `shift` must be all zeros here, see include/ryolo.h: the statistics include the padded rows of the
    last pixel tile, which are zeros only without a bias); returns the partial sums (fp64) [rows, 2, cpad] of z and z^2.
    clear=False: the caller guarantees the scratch is zero (bn_finalize zeroes what it read, so a scratch that started
    zeroed stays clean from conv to conv)."""
    L = _lib.lib()
    rows = L.ryolo_conv_stat_rows(C.byref(d))
    cp = cpad(d.Cout)
    if part is None:
        part = torch.zeros((rows, 2, cp), dtype=torch.float64, device=x.device)
    else:                       # caller-owned scratch (any shape with enough elements): carve [rows, 2, cp]
        part = part.view(-1)[:rows * 2 * cp].view(rows, 2, cp)
        if clear:
            part.zero_()
    if z is not None:
        d.out_cstride = _check_nhwc(z, "z")
    # z = None: statistics only (layer 0 of the training engine: conv0_recompute_supported(d); z is recomputed, never stored)
    _lib.check(L.ryolo_conv2d_bn_act_stats(C.byref(d), x.data_ptr(), packed_w.data_ptr(), ones.data_ptr(), shift.data_ptr(),
                                           None, z.data_ptr() if z is not None else None, part.data_ptr(), _s(x.device)),
               "ryolo_conv2d_bn_act_stats")
    return part


def conv0_recompute_supported(d):
    """Layer 0 (3x3 / stride 1 / pad 1, 8 padded input channels -> 32): train without storing the conv output (include/ryolo.h)."""
    return bool(_lib.lib().ryolo_conv0_recompute_supported(C.byref(d)))


def conv0_bn_act_fwd(d, x, packed_w, scale, shift, act, slope, y):
    """y = act(conv(x, W) * scale + shift), batch statistics already folded into scale / shift; slope: device scalar (PReLU)."""
    d.out_cstride = _check_nhwc(y, "y")
    _lib.check(_lib.lib().ryolo_conv0_bn_act_fwd(C.byref(d), x.data_ptr(), packed_w.data_ptr(), scale.data_ptr(), shift.data_ptr(), act,
                                                 slope.data_ptr() if slope is not None else None, y.data_ptr(), _s(x.device)),
               "ryolo_conv0_bn_act_fwd")
    return y


def conv0_bn_bwd_ws(device):
    """zeroed workspace of conv0_bn_bwd (the call leaves it zeroed)"""
    return torch.zeros(_lib.lib().ryolo_conv0_bn_bwd_workspace_bytes(), dtype=torch.uint8, device=device)


def conv0_bn_bwd(d, x, packed_w, dy, stats, act, slope, dz, dgamma, dbeta, dslope, ws, ws_is_zero=True):
    """bn_act_bwd for layer 0 with z recomputed from x in both passes (no stored conv output)."""
    mean, invstd, scale, shift = stats
    _lib.check(_lib.lib().ryolo_conv0_bn_bwd(C.byref(d), x.data_ptr(), packed_w.data_ptr(), dy.data_ptr(), dy.stride(2),
                                             scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), act,
                                             slope.data_ptr() if slope is not None else None, dz.data_ptr(), dz.stride(2),
                                             dgamma.data_ptr(), dbeta.data_ptr(), dslope.data_ptr() if dslope is not None else None,
                                             ws.data_ptr(), ws.numel(), 1 if ws_is_zero else 0, _s(x.device)), "ryolo_conv0_bn_bwd")
    return dz


def conv0_bn_bwd_wgrad_ws(device):
    return torch.empty(_lib.lib().ryolo_conv0_bn_bwd_wgrad_workspace_bytes(), dtype=torch.uint8, device=device)


def conv0_bn_bwd_wgrad(d, x, packed_w, dy, stats, act, slope, dgamma, dbeta, dslope, grad_w, cin_real, accumulate, ws):
    """Layer 0's whole backward in one pass over dy (csrc/conv0_bwd.hip): dgamma / dbeta / dslope and the conv's weight gradient
    (OIHW fp32, the `cin_real` real input channels) without materialising dz."""
    mean, invstd, scale, shift = stats
    _lib.check(_lib.lib().ryolo_conv0_bn_bwd_wgrad(C.byref(d), x.data_ptr(), packed_w.data_ptr(), dy.data_ptr(), dy.stride(2),
                                                   scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), act,
                                                   slope.data_ptr() if slope is not None else None, dgamma.data_ptr(), dbeta.data_ptr(),
                                                   dslope.data_ptr() if dslope is not None else None, grad_w.data_ptr(), int(cin_real),
                                                   1 if accumulate else 0, ws.data_ptr(), ws.numel(), _s(x.device)), "ryolo_conv0_bn_bwd_wgrad")


def conv_fwd_plain(d, x, packed_w, ones, shift, z):
    """z = conv(x, W) + shift (linear), no statistics (the bias convs in front of the yolo layers)."""
    d.out_cstride = _check_nhwc(z, "z")
    _lib.check(_lib.lib().ryolo_conv2d_bn_act(C.byref(d), x.data_ptr(), packed_w.data_ptr(), ones.data_ptr(), shift.data_ptr(),
                                              None, z.data_ptr(), _s(x.device)), "ryolo_conv2d_bn_act")


def conv_head_decode_store(hf, x, packed_w, ones, shift, head, p):
    """A YOLO head of the training forward in one launch: head = conv(x, W) + shift (NHWC bf16, what conv_fwd_plain stores) and
    p [bs, na, ny, nx, no] fp32, the raw rows ryolo_yolo_decode hands out.  hf: dict(desc, na, no) of plan.plan_train."""
    d = ConvDesc(*hf['desc'])
    d.in_cstride = _check_nhwc(x, "x")
    hcs = _check_nhwc(head, "head")
    if not p.is_contiguous() or p.dtype != torch.float32:
        raise ValueError("conv_head_decode_store: p must be contiguous fp32")
    _lib.check(_lib.lib().ryolo_conv_head_decode_store(C.byref(d), x.data_ptr(), packed_w.data_ptr(), ones.data_ptr(), shift.data_ptr(),
                                                       hf['na'], hf['no'], head.data_ptr(), hcs, p.data_ptr(), _s(x.device)),
               "ryolo_conv_head_decode_store")


def bn_finalize(part, C_, count, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, out=None):
    dev = part.device
    if out is None:
        out = [torch.empty(C_, dtype=torch.float32, device=dev) for _ in range(4)]      # mean, invstd, scale, shift
    _lib.check(_lib.lib().ryolo_bn_finalize(part.data_ptr(), part.shape[0], part.shape[2], C_, int(count), eps, momentum,
                                            gamma.data_ptr(), beta.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                            out[2].data_ptr(), out[3].data_ptr(),
                                            running_mean.data_ptr() if running_mean is not None else None,
                                            running_var.data_ptr() if running_var is not None else None, _s(dev)),
               "ryolo_bn_finalize")
    return out


def bn_act_fwd(z, scale, shift, act, slope, y, residual=None):
    n, h, w, c = z.shape
    _lib.check(_lib.lib().ryolo_bn_act_fwd(z.data_ptr(), z.stride(2), scale.data_ptr(), shift.data_ptr(), act,
                                           slope.data_ptr() if slope is not None else None,
                                           residual.data_ptr() if residual is not None else None,
                                           residual.stride(2) if residual is not None else 0, y.data_ptr(), y.stride(2),
                                           n * h * w, c, _s(z.device)), "ryolo_bn_act_fwd")
    return y


def bn_act_bwd(z, dy, stats, act, slope, dz, dgamma, dbeta, dslope, ws):
    """stats = (mean, invstd, scale, shift) or None for a bias conv (then only dbeta (= dbias) is accumulated)."""
    n, h, w, c = z.shape
    mean, invstd, scale, shift = stats if stats is not None else (None, None, None, None)
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    _lib.check(_lib.lib().ryolo_bn_act_bwd(z.data_ptr(), z.stride(2), dy.data_ptr(), dy.stride(2), p(scale), p(shift), p(mean),
                                           p(invstd), act, p(slope), p(dz), dz.stride(2) if dz is not None else 0,
                                           n * h * w, c, p(dgamma), p(dbeta), p(dslope), ws.data_ptr(), ws.numel(),
                                           _s(z.device)), "ryolo_bn_act_bwd")


def bn_bwd_ws_bytes(npix, c):
    return _lib.lib().ryolo_bn_act_bwd_workspace_bytes(npix, c)


_tap_tables = {}


def dgrad_tap_table(ksize, stride, device):
    key = (ksize, stride, device.index)
    t = _tap_tables.get(key)
    if t is None:
        host = (C.c_int * 72)()
        _lib.check(_lib.lib().ryolo_conv_dgrad_tap_table(ksize, stride, host), "ryolo_conv_dgrad_tap_table")
        t = torch.tensor(list(host), dtype=torch.int32, device=device)
        _tap_tables[key] = t
    return t


def pack_weights_dgrad(weight, stride, out=None):
    cout, cin, k, _ = weight.shape
    L = _lib.lib()
    nbytes = L.ryolo_conv_packed_dgrad_bytes(cout, cin, k, stride)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    w = weight.contiguous()
    table = dgrad_tap_table(k, stride, weight.device)
    _lib.check(L.ryolo_conv_pack_weights_dgrad(w.data_ptr(), cout, cin, k, stride, out.data_ptr(), table.data_ptr(),
                                               _s(weight.device)), "ryolo_conv_pack_weights_dgrad")
    return out


def conv_dgrad(d, dz, packed_dgrad, ones, zeros, dx, accumulate):
    _lib.check(_lib.lib().ryolo_conv2d_dgrad(C.byref(d), dz.data_ptr(), dz.stride(2), packed_dgrad.data_ptr(), ones.data_ptr(),
                                             zeros.data_ptr(), dx.data_ptr(), 1 if accumulate else 0, _s(dz.device)),
               "ryolo_conv2d_dgrad")


def dgrad_bnreduce_rows(d):
    """rows of partial sums conv_dgrad_bnreduce writes for this (forward) conv, 0 = its data gradient cannot carry the reduce"""
    return _lib.lib().ryolo_conv2d_dgrad_bnreduce_rows(C.byref(d))


def conv_dgrad_bnreduce(d, dz, packed_dgrad, ones, zeros, dx, accumulate, z, stats, slope, part):
    """conv_dgrad that also runs the reduce pass of the BatchNorm/PReLU backward of the block that produced this conv's input
    (z = that block's conv output, stats = its (mean, invstd, scale, shift)) on the final dx: part [rows, 3, C_in] fp32."""
    mean, invstd, scale, shift = stats
    _lib.check(_lib.lib().ryolo_conv2d_dgrad_bnreduce(C.byref(d), dz.data_ptr(), dz.stride(2), packed_dgrad.data_ptr(), ones.data_ptr(),
                                                      zeros.data_ptr(), dx.data_ptr(), 1 if accumulate else 0, z.data_ptr(), z.stride(2),
                                                      scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                                      slope.data_ptr(), part.data_ptr(), _s(dz.device)), "ryolo_conv2d_dgrad_bnreduce")


def bn_act_bwd_reduced(z, dy, stats, act, slope, dz, dgamma, dbeta, dslope, part, ws):
    """bn_act_bwd whose reduce pass already ran inside conv_dgrad_bnreduce (part [rows, 3, C]); ws: >= 3*C floats."""
    n, h, w, c = z.shape
    mean, invstd, scale, shift = stats
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    _lib.check(_lib.lib().ryolo_bn_act_bwd_reduced(z.data_ptr(), z.stride(2), dy.data_ptr(), dy.stride(2), scale.data_ptr(), shift.data_ptr(),
                                                   mean.data_ptr(), invstd.data_ptr(), act, p(slope), dz.data_ptr(), dz.stride(2), n * h * w, c,
                                                   p(dgamma), p(dbeta), p(dslope), part.data_ptr(), part.shape[0], ws.data_ptr(), ws.numel(),
                                                   _s(z.device)), "ryolo_bn_act_bwd_reduced")


def wgrad_ws_bytes(d):
    return _lib.lib().ryolo_conv_wgrad_workspace_bytes(C.byref(d))


def conv_wgrad(d, x, dz, cin_real, grad, accumulate, ws):
    L = _lib.lib()
    args = (C.byref(d), x.data_ptr(), dz.data_ptr(), dz.stride(2), cin_real, grad.data_ptr(), 1 if accumulate else 0, ws.data_ptr(),
            ws.numel(), _s(x.device))
    if isinstance(L, _lib._CallTracer):          # bench.py's traced steps: the tile kernel and the split-K reduce as two timed calls
        _lib.check(L.ryolo_conv2d_wgrad_partials(*args), "ryolo_conv2d_wgrad_partials")
        _lib.check(L.ryolo_conv2d_wgrad_reduce(*args), "ryolo_conv2d_wgrad_reduce")
        return
    _lib.check(L.ryolo_conv2d_wgrad(*args), "ryolo_conv2d_wgrad")


def conv_wgrad_partials(d, x, dz, cin_real, grad, accumulate, ws):
    """the tile kernel of conv_wgrad only: the layer's split-K partial tiles stay in `ws` for a later (batched) reduce"""
    _lib.check(_lib.lib().ryolo_conv2d_wgrad_partials(C.byref(d), x.data_ptr(), dz.data_ptr(), dz.stride(2), cin_real, grad.data_ptr(),
                                                      1 if accumulate else 0, ws.data_ptr(), ws.numel(), _s(x.device)),
               "ryolo_conv2d_wgrad_partials")


# ---- the dilated shared 3x3 conv of the matrix cfgs (signatures: _lib.py)
def _dil(dil):
    dh, dw = (dil, dil) if isinstance(dil, int) else dil
    return int(dh), int(dw)


def dilated_desc(n, h, w, cin, cout, in_cs=None, out_cs=None):
    """the forward descriptor of a dilated 3x3 / stride 1 conv (include/ryolo.h: ksize 3, pad 1 names the undilated window)"""
    return ConvDesc(n, h, w, cin, cout, 3, 1, 1, in_cs or cin, out_cs or cout, 0, 0, 0.0, 1, 0)


def conv_dilated_dgrad_supported(d, dil):
    return bool(_lib.lib().ryolo_conv2d_dilated_dgrad_supported(C.byref(d), *_dil(dil)))


def conv_dilated_wgrad_supported(d, dil):
    return bool(_lib.lib().ryolo_conv2d_dilated_wgrad_supported(C.byref(d), *_dil(dil)))


def conv_dilated_wgrad_ws_bytes(d, dil):
    return _lib.lib().ryolo_conv2d_dilated_wgrad_workspace_bytes(C.byref(d), *_dil(dil))


def conv_dilated_dgrad(d, dil, dz, packed_dgrad, ones, zeros, dx):
    """dx = conv3x3(dz, flipped / transposed W, padding=dil, dilation=dil) for the FORWARD conv `d` (csrc/conv_dil.hip); packed_dgrad: the
    stride-1 image of pack_weights_dgrad for the shared weight; ones / zeros: fp32 [cpad(Cin)]"""
    _check_nhwc(dz, "dz")
    _check_nhwc(dx, "dx")
    dh, dw = _dil(dil)
    with torch.cuda.device(dz.device):
        rc = _lib.lib().ryolo_conv2d_dilated_dgrad(C.byref(d), dh, dw, dz.data_ptr(), dz.stride(2), packed_dgrad.data_ptr(), ones.data_ptr(),
                                                   zeros.data_ptr(), dx.data_ptr(), _s(dz.device))
    _lib.check(rc, "ryolo_conv2d_dilated_dgrad")


def conv_dilated_wgrad(d, dil, x, dz, grad, accumulate, ws):
    """grad (fp32 OIHW) (+)= the weight gradient of the dilated conv `d` (csrc/wgrad_dil.hip); ws: uint8, >= conv_dilated_wgrad_ws_bytes"""
    _check_nhwc(x, "x")
    _check_nhwc(dz, "dz")
    dh, dw = _dil(dil)
    with torch.cuda.device(x.device):
        rc = _lib.lib().ryolo_conv2d_dilated_wgrad(C.byref(d), dh, dw, x.data_ptr(), dz.data_ptr(), dz.stride(2), grad.data_ptr(),
                                                   1 if accumulate else 0, ws.data_ptr(), ws.numel() * ws.element_size(), _s(x.device))
    _lib.check(rc, "ryolo_conv2d_dilated_wgrad")


class SharedConvPacks(object):
    """The packed images of the shared source weights of one model, forward and data-gradient, keyed on the weight's (data_ptr, _version):
    the sharers of a source pack it once per direction per optimizer step (an in-place update bumps the version).  Also holds the per-channel
    ones / zeros vectors the kernels' epilogue reads.  Lives on the model (Darknet.shared_conv_packs)."""

    def __init__(self):
        self._fwd, self._dgrad, self._vec = {}, {}, {}

    @staticmethod
    def _get(table, weight, pack):
        ent = table.get(weight.data_ptr())
        if ent is None or ent[0] != weight._version:
            ent = (weight._version, pack(weight))
            table[weight.data_ptr()] = ent
        return ent[1]

    def forward_image(self, weight):
        return self._get(self._fwd, weight, lambda w: pack_weights(w.detach()))

    def dgrad_image(self, weight):
        return self._get(self._dgrad, weight, lambda w: pack_weights_dgrad(w.detach(), 1))

    def vectors(self, c, device):
        """(ones, zeros) fp32 [cpad(c)]"""
        key = (cpad(c), device.index)
        v = self._vec.get(key)
        if v is None:
            v = (torch.ones(key[0], dtype=torch.float32, device=device), torch.zeros(key[0], dtype=torch.float32, device=device))
            self._vec[key] = v
        return v


class SharedDilatedConv(torch.autograd.Function):
    """y = F.conv2d(x, weight, padding=dil, dilation=dil) for a d-convolutional block with weight_from (model/models.py:254-267) on the HIP
    kernels, inside an ATen chain: x NCHW fp32 -> NHWC bf16, ryolo_conv2d_dilated (scale 1, shift 0, linear), -> NCHW fp32.  Saves the bf16
    NHWC x, not the fp32 input.  Backward: dy -> NHWC bf16; the data gradient only when the input needs one; the weight gradient into a
    fresh fp32 OIHW tensor that is returned -- autograd sums the sharers.  apply(x, weight, dil[, packs]): packs = the model's
    SharedConvPacks (None: pack for this call)."""

    @staticmethod
    def forward(ctx, x, weight, dil, packs=None):
        packs = packs if packs is not None else SharedConvPacks()
        cout, cin = weight.shape[0], weight.shape[1]
        xb = hip_ops.nchw_f32_to_nhwc_bf16(x)
        ones, zeros = packs.vectors(cout, x.device)
        yb = hip_ops.conv2d_dilated(xb, packs.forward_image(weight), ones, zeros, cout, dil)
        ctx.save_for_backward(xb, weight)
        ctx.dil, ctx.packs = _dil(dil), packs
        return hip_ops.nhwc_bf16_to_nchw_f32(yb)

    @staticmethod
    def backward(ctx, dy):
        xb, weight = ctx.saved_tensors
        n, h, w, cin = xb.shape
        cout = weight.shape[0]
        d = dilated_desc(n, h, w, cin, cout)
        dyb = hip_ops.nchw_f32_to_nhwc_bf16(dy.float())
        dx = dw = None
        if ctx.needs_input_grad[0]:
            ones, zeros = ctx.packs.vectors(cin, dy.device)
            dxb = torch.empty((n, h, w, cin), dtype=torch.bfloat16, device=dy.device)
            conv_dilated_dgrad(d, ctx.dil, dyb, ctx.packs.dgrad_image(weight), ones, zeros, dxb)
            dx = hip_ops.nhwc_bf16_to_nchw_f32(dxb)
        if ctx.needs_input_grad[1]:
            dw = torch.empty(weight.shape, dtype=torch.float32, device=dy.device)
            ws = torch.empty(conv_dilated_wgrad_ws_bytes(d, ctx.dil), dtype=torch.uint8, device=dy.device)
            conv_dilated_wgrad(d, ctx.dil, xb, dyb, dw, False, ws)
        return dx, dw, None, None


# ---- squeeze-and-excitation backward (csrc/se_bwd.hip; signatures: _lib.py)
def se_bwd_ws_bytes(n, h, w, c, hidden):
    """bytes of scratch of one se_bwd_nhwc call; 0: the shape is not served (no device call)"""
    return _lib.lib().ryolo_se_bwd_workspace_bytes(int(n), int(h), int(w), int(c), int(hidden))


def se_bwd_nhwc(x, dy, w1, w2, dx=None, dw1=None, dw2=None, dx_accumulate=False, accumulate_w=False, gate_out=None, workspace=None):
    """The gradients of y = x * sigmoid(W2 . relu(W1 . mean_hw(x))) given dy (include/ryolo.h: ryolo_se_bwd_nhwc).  x, dy, dx: NHWC bf16
    (possibly slices); w1 [hidden, C], w2 [C, hidden], dw1, dw2: contiguous fp32; dx None: no data gradient; dw1 and dw2 None: no weight
    gradients; gate_out: fp32 [N, C] that receives the recomputed gates; workspace: uint8, >= se_bwd_ws_bytes (None: allocated here)."""
    x_cs = _check_nhwc(x, "x")
    dy_cs = _check_nhwc(dy, "dy")
    n, h, w, c = x.shape
    assert tuple(dy.shape) == (n, h, w, c), (tuple(dy.shape), (n, h, w, c))
    hidden = w1.shape[0]
    for t, shape, name in ((w1, (hidden, c), "w1"), (w2, (c, hidden), "w2"), (dw1, (hidden, c), "dw1"), (dw2, (c, hidden), "dw2"),
                           (gate_out, (n, c), "gate_out")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError("%s must be a contiguous fp32 GPU tensor of shape %s" % (name, shape))
    dx_cs = 0
    if dx is not None:
        dx_cs = _check_nhwc(dx, "dx")
        assert tuple(dx.shape) == (n, h, w, c), (tuple(dx.shape), (n, h, w, c))
    if workspace is None:
        nbytes = se_bwd_ws_bytes(n, h, w, c, hidden)
        if nbytes == 0:
            raise RuntimeError("se backward: unsupported shape N %d, H %d, W %d, C %d, hidden %d (C a multiple of 8 from 16 to 2048, "
                               "hidden from 1 to 128)" % (n, h, w, c, hidden))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)

    def ptr(t):
        return t.data_ptr() if t is not None else None
    with torch.cuda.device(x.device):
        rc = _lib.lib().ryolo_se_bwd_nhwc(x.data_ptr(), x_cs, dy.data_ptr(), dy_cs, w1.data_ptr(), w2.data_ptr(), hidden, ptr(dx), dx_cs,
                                          1 if dx_accumulate else 0, ptr(dw1), ptr(dw2), 1 if accumulate_w else 0, n, h, w, c,
                                          ptr(gate_out), workspace.data_ptr(), workspace.numel() * workspace.element_size(), _s(x.device))
    _lib.check(rc, "ryolo_se_bwd_nhwc")
    return dx


def se_supported(n, h, w, c, hidden):
    """do csrc/se.hip and csrc/se_bwd.hip serve this block (no device call)"""
    return _lib.lib().ryolo_se_workspace_bytes(int(n), int(h), int(w), int(c)) > 0 and se_bwd_ws_bytes(n, h, w, c, hidden) > 0


class SqueezeExcite(torch.autograd.Function):
    """y = x * sigmoid(W2 . relu(W1 . mean_hw(x))) -- SELayer.forward (model/models.py:27-31) on the HIP kernels, inside an ATen chain:
    x NCHW fp32 -> NHWC bf16, ryolo_se_nhwc, -> NCHW fp32.  Saves the bf16 NHWC x and the two weights, not the gate (the backward
    recomputes it).  Backward: dy -> NHWC bf16, one ryolo_se_bwd_nhwc call -- the data gradient only when the input needs one, the weight
    gradients only when a weight needs one -- into fresh fp32 tensors; scratch from torch's allocator per call.  apply(x, w1, w2) with
    w1 = fc.0.weight [C/16, C], w2 = fc.2.weight [C, C/16].  A CPU tensor raises: there is no fallback."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        if not (x.is_cuda and w1.is_cuda and w2.is_cuda):
            raise RuntimeError("SqueezeExcite runs on the HIP kernels: x, w1 and w2 must be GPU tensors")
        if x.shape[1] % 8:
            raise RuntimeError("SqueezeExcite: %d channels (the kernels need a multiple of 8)" % x.shape[1])
        xb = hip_ops.nchw_f32_to_nhwc_bf16(x.float())
        w1c, w2c = w1.detach().float().contiguous(), w2.detach().float().contiguous()
        yb = hip_ops.se_nhwc(xb, w1c, w2c)
        ctx.save_for_backward(xb, w1c, w2c)
        return hip_ops.nhwc_bf16_to_nchw_f32(yb)

    @staticmethod
    def backward(ctx, dy):
        xb, w1, w2 = ctx.saved_tensors
        dyb = hip_ops.nchw_f32_to_nhwc_bf16(dy.float())
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (need_x or need_w):
            return None, None, None
        dxb = torch.empty_like(xb) if need_x else None
        dw1 = torch.empty_like(w1) if need_w else None
        dw2 = torch.empty_like(w2) if need_w else None
        se_bwd_nhwc(xb, dyb, w1, w2, dx=dxb, dw1=dw1, dw2=dw2)
        dx = hip_ops.nhwc_bf16_to_nchw_f32(dxb) if need_x else None
        return dx, (dw1 if ctx.needs_input_grad[1] else None), (dw2 if ctx.needs_input_grad[2] else None)


def upsample2x_bwd(dy, dx, accumulate):
    n, h, w, c = dx.shape
    _lib.check(_lib.lib().ryolo_upsample2x_bwd(dy.data_ptr(), dy.stride(2), dx.data_ptr(), dx.stride(2), n, h, w, c,
                                               1 if accumulate else 0, _s(dy.device)), "ryolo_upsample2x_bwd")


def pgrad_to_nhwc(pgrad, out):
    bs, na, ny, nx, no = pgrad.shape
    g = pgrad.contiguous()
    _lib.check(_lib.lib().ryolo_pgrad_to_nhwc(g.data_ptr(), bs, na, ny, nx, no, out.data_ptr(), out.stride(2), _s(g.device)),
               "ryolo_pgrad_to_nhwc")


def yolo_loss_bitmap(p, nc=1, arc=0):
    """Zeroed dedup bitmap for ryolo_yolo_loss[_arc] on head tensor p [bs, na, ny, nx, no]."""
    cells = p.numel() // p.shape[-1]
    return torch.zeros(_lib.lib().ryolo_yolo_loss_bitmap_bytes_arc(cells, nc, arc) // 4, dtype=torch.int32, device=p.device)


def yolo_loss_head(p, hd, nc, h, bitmap, dp, items, arc=0):
    """One head of the 'default'-arc loss + gradient (csrc/loss.hip).  hd: a dict from loss_static.build_targets_static
    (w, b, gj, gi, cls, gxy, gwh, ga, av); h: hyper-parameters; bitmap zeroed by the caller; items[0..2] accumulated."""
    bs, na, ny, nx, no = p.shape
    w = hd['w'].contiguous()
    n = hd['npos'] if 'npos' in hd else w.sum()
    c = lambda t: t.contiguous()   # noqa: E731
    b, gj, gi, cls = c(hd['b']), c(hd['gj']), c(hd['gi']), c(hd['cls'])
    txy, twh, ta, av = c(hd['gxy']), c(hd['gwh']), c(hd['ga']), c(hd['av'].float())
    _lib.check(_lib.lib().ryolo_yolo_loss_arc(p.data_ptr(), bs, na, ny, nx, no, nc, w.data_ptr(), w.shape[1], b.data_ptr(),
                                              gj.data_ptr(), gi.data_ptr(), cls.data_ptr(), txy.data_ptr(), twh.data_ptr(),
                                              ta.data_ptr(), av.data_ptr(), n.data_ptr(), float(h['giou']), float(h['reg']),
                                              float(h['cls']), float(h['cls_pw']), float(h['obj']), float(h['obj_pw']),
                                              1 if h.get('riou', 0) else 0, int(arc), float(h.get('fl_gamma', 0.0)),
                                              bitmap.data_ptr(), dp.data_ptr(), items.data_ptr(), _s(p.device)),
               "ryolo_yolo_loss_arc")


def yolo_loss_head_nhwc(head, p, hd, nc, h, bitmap, dp_sparse, head_g, items, arc=0, bias_part=None):
    """yolo_loss_head for a head of the training engine: `head` / `head_g` are the NHWC bf16 activation and gradient buffers of
    the head conv, dp_sparse an all-zero fp32 scratch shaped like p (left all-zero); see ryolo_yolo_loss_nhwc.
    bias_part ([yolo_loss_bias_rows(p, arc), >= C] fp32, or None): the dense pass also writes rows of partial sums of the head
    conv's bias gradient (head_bias_finalize turns them into dbias)."""
    bs, na, ny, nx, no = p.shape
    w = hd['w'].contiguous()
    n = hd['npos'] if 'npos' in hd else w.sum()
    c = lambda t: t.contiguous()   # noqa: E731
    b, gj, gi, cls = c(hd['b']), c(hd['gj']), c(hd['gi']), c(hd['cls'])
    txy, twh, ta, av = c(hd['gxy']), c(hd['gwh']), c(hd['ga']), c(hd['av'].float())
    if bias_part is not None and (bias_part.dtype != torch.float32 or not bias_part.is_contiguous()
                                  or bias_part.shape[0] != yolo_loss_bias_rows(p, arc)):
        raise ValueError("yolo_loss_head_nhwc: bias_part must be contiguous fp32 [yolo_loss_bias_rows, >= C]")
    _lib.check(_lib.lib().ryolo_yolo_loss_nhwc_bias(head.data_ptr(), head.stride(2), p.data_ptr(), bs, na, ny, nx, no, nc, w.data_ptr(),
                                                    w.shape[1], b.data_ptr(), gj.data_ptr(), gi.data_ptr(), cls.data_ptr(),
                                                    txy.data_ptr(), twh.data_ptr(), ta.data_ptr(), av.data_ptr(), n.data_ptr(),
                                                    float(h['giou']), float(h['reg']), float(h['cls']), float(h['cls_pw']),
                                                    float(h['obj']), float(h['obj_pw']), 1 if h.get('riou', 0) else 0, int(arc),
                                                    float(h.get('fl_gamma', 0.0)), bitmap.data_ptr(), dp_sparse.data_ptr(),
                                                    head_g.data_ptr(), head_g.stride(2), items.data_ptr(),
                                                    bias_part.data_ptr() if bias_part is not None else None,
                                                    bias_part.shape[1] if bias_part is not None else 0, _s(p.device)),
               "ryolo_yolo_loss_nhwc_bias")


def yolo_loss_bias_rows(p, arc=0):
    """rows of bias partial sums the dense pass of yolo_loss_head_nhwc writes for head p [bs, na, ny, nx, no]; 0: fold not served"""
    bs, na, ny, nx, no = p.shape
    return _lib.lib().ryolo_yolo_loss_bias_rows(bs, na, ny, nx, no, int(arc))


def head_bias_ws_bytes(npix, c):
    return _lib.lib().ryolo_head_bias_workspace_bytes(npix, c)


def head_bias_finalize(bias_part, npix, c, g, dbias, ws):
    """dbias[:c] += g[0] * sum over the rows of bias_part, in the order bn_act_bwd's bias form sums the [npix, c] head gradient (for
    g == 1: the same bits)"""
    _lib.check(_lib.lib().ryolo_head_bias_finalize(bias_part.data_ptr(), npix, bias_part.shape[1], c, g.data_ptr(),
                                                   dbias.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _s(dbias.device)),
               "ryolo_head_bias_finalize")


def scale_bf16_if(g, buf):
    """buf (NHWC bf16) *= g[0] unless g[0] == 1, decided on the device."""
    n, hh, ww, cc = buf.shape
    _lib.check(_lib.lib().ryolo_scale_bf16_if(g.data_ptr(), buf.data_ptr(), buf.stride(2), n * hh * ww, cc, _s(buf.device)),
               "ryolo_scale_bf16_if")


class RotatedIoU(torch.autograd.Function):
    """iou[n] = rotated IoU(pbox[n,5], tbox[n,5]) with the polygon-overlap gradient w.r.t. pbox (csrc/riou_grad.h); tbox is
    a constant.  CUDA fp32 tensors only -- there is no CPU path."""

    @staticmethod
    def forward(ctx, pbox, tbox):
        if not pbox.is_cuda:
            raise RuntimeError("RotatedIoU runs on the HIP kernel only (got a CPU tensor)")
        p = pbox.detach().float().contiguous()
        t = tbox.detach().float().contiguous()
        n = p.shape[0]
        iou = torch.empty(n, dtype=torch.float32, device=p.device)
        grad = torch.empty(n, 5, dtype=torch.float32, device=p.device)
        _lib.check(_lib.lib().ryolo_riou_loss_pairs(p.data_ptr(), t.data_ptr(), n, iou.data_ptr(), grad.data_ptr(), _s(p.device)),
                   "ryolo_riou_loss_pairs")
        ctx.save_for_backward(grad)
        return iou

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g.unsqueeze(1), None


class BuildTargets(object):
    """build_targets for all heads in one launch (csrc/loss.hip), writing into static buffers; `heads()` returns the dicts
    loss_static.build_targets_static returns (views of those buffers), `npos[h]` the positives' count."""

    def __init__(self, core, capacity, device):
        self.NT, self.dev = int(capacity), device
        self.layers = [core.module_list[i] for i in core.yolo_layers]
        self.nh, self.na = len(self.layers), int(self.layers[0].anchor_vec.shape[0])
        f32 = dict(dtype=torch.float32, device=device)
        self.ng = [l.ng.to(**f32).contiguous() for l in self.layers]
        self.av = [l.anchor_vec.to(**f32).contiguous() for l in self.layers]
        self.w = [torch.zeros(self.na, self.NT, **f32) for _ in self.layers]
        self.idx = [torch.zeros(4, self.NT, dtype=torch.int64, device=device) for _ in self.layers]
        self.box = [torch.zeros(5 * self.NT, **f32) for _ in self.layers]
        self.npos = torch.zeros(self.nh, **f32)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
        self._ptrs = [arr(self.ng), arr(self.av), arr(self.w), arr(self.idx), arr(self.box),
                      arr([self.npos[h:h + 1] for h in range(self.nh)])]

    def run(self, tpad, valid, h, context_factor):
        self.npos.zero_()
        p = self._ptrs
        _lib.check(_lib.lib().ryolo_build_targets(tpad.data_ptr(), valid.data_ptr(), self.NT, self.nh, self.na, p[0], p[1],
                                                  float(h['iou_t']), float(h['ang_t']), float(context_factor), p[2], p[3], p[4],
                                                  p[5], _s(self.dev)), "ryolo_build_targets")

    def heads(self):
        NT = self.NT
        return [dict(w=self.w[k], b=self.idx[k][0], cls=self.idx[k][1], gj=self.idx[k][2], gi=self.idx[k][3],
                     gxy=self.box[k][:2 * NT].view(NT, 2), gwh=self.box[k][2 * NT:4 * NT].view(NT, 2), ga=self.box[k][4 * NT:],
                     av=self.av[k], npos=self.npos[k:k + 1]) for k in range(self.nh)]
