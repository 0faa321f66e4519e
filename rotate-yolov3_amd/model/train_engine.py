"""TrainEngine -- forward + backward of the Darknet cfg graph in TRAINING mode on the hand-written HIP kernels.

Replaces, for `model.train(); pred = model(imgs); loss.backward()` (train.py:268-282), the autograd walk over
nn.Conv2d / nn.BatchNorm2d (batch statistics, per replica) / nn.PReLU / shortcut / route / upsample that the reference
dispatches to cuDNN/ATen.  The engine returns the head tensors `p` as outputs of an autograd Function and receives
dL/dp back -- from the eager loss mirror (model/loss.py) or, with Darknet.enable_fused_loss(), from the graph-captured
HIP loss (model/loss_static.py, csrc/loss.hip), which writes the engine's head-gradient buffers directly.

Forward per `convolutional` block:   z = conv(x, W) (+ per-channel sums of z, z^2 in the conv epilogue)
                                     -> bn_finalize (mean, invstd, running stats, folded scale/shift)
                                     -> y = PReLU(z*scale + shift) [+ shortcut source]            (bn_act_fwd)
Backward per block:                  dy -> bn_act_bwd -> dz, dgamma, dbeta, dslope
                                     dW += wgrad(x, dz);   dx (+)= dgrad(dz, W)
Saved for backward: x (the producer's output, never overwritten), z, the four per-channel statistics.
Gradient buffers mirror the activation buffers (same concat/slice structure); the FIRST contribution to a gradient
view overwrites it and later ones accumulate (decided statically at plan time, no memset of the 6 GB of gradients).
Residual chains share ONE gradient buffer per stage (the skip branch receives dy unchanged, so no copy).
Parameter gradients accumulate in one flat fp32 buffer with stable addresses and are added to `param.grad` (possibly
views of the data-parallel buckets of rotate-yolov3_amd/dist.py) segment by segment: the backward launch list is cut
where a bucket has received its last gradient and the reducer's hooks run there, so buckets travel during backward.
Forward and each backward segment are replayed from hipGraphs after two eager steps.  Packed bf16 weight images
(forward layout and every dgrad class) are rebuilt from the fp32 parameters each step by ONE launch.

State is explicit: a conv block is a `ConvBlock` (slots, all assigned in its constructor), the other entries of the launch lists are
the planner's AddRec / UpRec with tensors for views and a `YoloEntry`; every engine attribute is assigned in `__init__`, which also
allocates what the forward needs.  What only a backward needs (head-gradient buffers, gradient sink, folded-reduce scratch, split-K
workspaces) is allocated by `_prepare_backward()`.  `_forward_launch` / `_backward_launch` -- the bodies the hipGraphs capture --
launch kernels and run in-place tensor operations, nothing else; they read the CURRENT parameter tensors (BatchNorm weight / bias /
running statistics, PReLU slope, conv bias), so an eager engine follows a replaced `.data`.
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

from .. import _lib
from . import hip_ops as ops
from . import hip_train_ops as tr
from . import plan
from .engine import HipEngine
from .models import create_grids
from .nhwc_batch import NHWC8Batch

# the engine's switches, read once when it is built.  RYOLO_NO_GRAPH=1 (bench.py --no-graph): eager launches from the start -- what a
# launcher falls back to when a runtime refuses stream capture under a multi-rank communicator (a failed capture also falls back by itself,
# see _capture); RYOLO_HEAD_DECODE=0 (the inference engine's switch): a YOLO head's conv and its decode stay two launches;
# RYOLO_HEAD_BIAS_FOLD=0: the head convs' bias gradients by the separate pass everywhere; RYOLO_WGRAD_BATCH_REDUCE=0: one split-K
# reduce launch behind every weight gradient, sharing one workspace; RYOLO_BN_REDUCE_FUSION=0: no BatchNorm reduce inside a data gradient
Switches = namedtuple('Switches', 'no_graph head_decode head_bias_fold batch_reduce bn_reduce_fusion')
# a yolo entry of TrainEngine.plan: head / head_g NHWC bf16 activation and gradient of the head conv, p [bs, na, ny, nx, no] fp32,
# io: scratch for the decoded rows or None, fused_block: the ConvBlock that runs conv + p rows + head store here as one launch, or None
YoloEntry = namedtuple('YoloEntry', 'head head_g module anchors p io ny nx fused_block')


class ConvBlock(object):
    """One `convolutional` block: the plan record's geometry, the engine's tensors for its views, the layer's modules and every constant
    its launches read.  Every slot is assigned here; None means "not applicable".
      i, desc, C, npix, cin_k, k, s, pad; xin, xin_g, y, dy, res, res_g, res_alias; z, dz: buffers of their own behind a BatchNorm (None:
          layer 0 recomputes z / its one-pass backward has no dz), else y and dy; recompute, bnbwd, dgrad, wgrad: what the plan says
      conv, bn, act (the PReLU / LeakyReLU or None), mish
      actcode, leaky (a LeakyReLU's slope on the device), stats (mean, invstd, scale, shift) -- BatchNorm blocks; bias_pad -- bias convs;
          packed, packed_d: the bf16 weight images; head_fused: dict(desc, na, no), the conv runs at its yolo entry; head_k: the head whose
          bias gradient the fused loss can supply
      backward only (TrainEngine._prepare_backward): ws_w, the split-K workspace of its own for the batched reduce; ws0, layer 0's
          workspace; red_for, the block whose BatchNorm reduce this block's data gradient runs, red_part, the rows left for this block"""
    __slots__ = ('i', 'desc', 'C', 'npix', 'cin_k', 'k', 's', 'pad', 'xin', 'xin_g', 'y', 'dy', 'res', 'res_g', 'res_alias', 'z', 'dz',
                 'recompute', 'bnbwd', 'dgrad', 'wgrad', 'conv', 'bn', 'act', 'mish', 'actcode', 'leaky', 'stats', 'bias_pad', 'packed',
                 'packed_d', 'head_fused', 'head_k', 'ws_w', 'ws0', 'red_for', 'red_part')

    def __init__(self, rec, m, tv, new_buf, device):
        L = _lib.lib()
        self.i = rec['layer']
        self.conv, self.bn = HipEngine._conv_of(m), HipEngine._bn_of(m)
        acts = [s_ for s_ in m if isinstance(s_, (nn.PReLU, nn.LeakyReLU))]
        self.act = acts[-1] if acts else None
        self.mish = any(type(s_).__name__ == 'Mish' for s_ in m)
        self.desc = ops.ConvDesc(*rec['desc'])
        self.k, self.s, self.pad = self.desc.ksize, self.desc.stride, self.desc.pad
        self.xin, self.xin_g, self.y, self.dy = tv(rec['xin']), tv(rec['xin_g']), tv(rec['y']), tv(rec['dy'])
        self.res, self.res_g, self.res_alias = tv(rec['res']), tv(rec['res_g']), rec['res_alias']
        self.C, h, w = rec['shape']
        self.npix, self.cin_k = self.xin.shape[0] * h * w, self.xin.shape[-1]
        self.recompute, self.bnbwd, self.dgrad, self.wgrad = rec['recompute'], rec['bnbwd'], rec['dgrad'], rec['wgrad']
        if self.bn is not None:
            self.z = None if rec['recompute'] else new_buf(*rec['shape'])
            # (layer 0's one-pass backward never materialises dz: 1.5 GB at bs 64 / 608^2)
            self.dz = None if (rec['one_pass'] or not rec['bnbwd']) else new_buf(*rec['shape'])
            self.stats = [torch.empty(self.C, dtype=torch.float32, device=device) for _ in range(4)]
            self.leaky = torch.full((1,), self.act.negative_slope, device=device) if isinstance(self.act, nn.LeakyReLU) else None
            self.actcode = 2 if self.mish else (1 if self.act is not None else 0)
            self.bias_pad = None
        else:
            self.z, self.dz = self.y, self.dy            # linear bias conv: y IS z, dz IS dy
            self.stats = self.leaky = self.actcode = None
            self.bias_pad = torch.zeros(ops.cpad(self.C), device=device) if self.conv.bias is not None else None
        wt = self.conv.weight
        if wt.dtype != torch.float32 or not wt.is_contiguous():
            raise RuntimeError("TrainEngine expects contiguous fp32 conv weights")
        cout, cin, k, _ = wt.shape
        self.packed = torch.empty(L.ryolo_conv_packed_weight_bytes(cout, self.cin_k, k), dtype=torch.uint8, device=device)
        self.packed_d = torch.empty(L.ryolo_conv_packed_dgrad_bytes(cout, cin, k, self.s), dtype=torch.uint8,
                                    device=device) if self.dgrad else None
        # a linear head conv the plan marked: conv + p rows + head-tensor store in one launch, issued at the yolo entry
        self.head_fused = rec['head_fused'] if self.act is None and not self.mish else None
        self.head_k = self.ws_w = self.ws0 = self.red_for = self.red_part = None

    @property
    def slope(self):
        """the activation's negative slope as a device tensor: the PReLU weight as it is NOW, the LeakyReLU constant, or None"""
        if self.bn is None:
            return None
        return self.act.weight.detach() if isinstance(self.act, nn.PReLU) else self.leaky

    @property
    def one_pass(self):
        """layer 0 when its whole backward is the one-pass kernel (csrc/conv0_bwd.hip: no dz, no separate weight gradient)"""
        return self.bn is not None and self.recompute and self.xin_g is None and self.dz is None

    @property
    def has_wgrad(self):
        return self.wgrad and not self.one_pass

    def bias_now(self, zeros):
        """the shift vector of a bias conv: bias_pad filled from the current Conv2d.bias, or `zeros` for a conv without bias"""
        if self.bias_pad is None:
            return zeros
        self.bias_pad[:self.C].copy_(self.conv.bias.detach())
        return self.bias_pad


class _Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, x, anchor):
        ctx.engine = engine
        outs = engine.forward(x)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.engine.backward(grads)
        return None, None, None


class TrainEngine(object):
    def __init__(self, model, x_shape, device, use_graph=True):
        _lib.lib()
        self.model = model

        def on(name):
            return os.environ.get(name, '1') != '0'
        sw = self.switches = Switches(os.environ.get('RYOLO_NO_GRAPH', '0') == '1', on('RYOLO_HEAD_DECODE'), on('RYOLO_HEAD_BIAS_FOLD'),
                                      on('RYOLO_WGRAD_BATCH_REDUCE'), on('RYOLO_BN_REDUCE_FUSION'))
        self.no_graph_env = sw.no_graph
        self.use_graph = use_graph and not sw.no_graph
        self.graph_fallback = None      # set when a hipGraph capture failed and the engine went back to eager launches
        self.reduce_fallback = None     # set when the batched split-K reduce's per-layer workspaces did not fit in memory
        self.force_eager = False        # measurement: launch eagerly although the graphs exist (bench.py's traced steps)
        self.backward_hook = None       # tests: called before / after every entry of the backward launch list (eager launches only)
        self.g_fwd = self.g_bwd = None
        self._segs = None
        self._red_planned = False
        self._warned_rebind = False
        self._fused_state = None        # the fused loss's per-engine capture state (model/loss_static.py)
        self.static_pg = None           # fp32 head-gradient buffers shaped like self.p: head_grad_buffers()
        self.steps = 0
        self.device = device
        self.bs, cin, self.H, self.W = [int(v) for v in x_shape]
        defs, mods = model.module_defs, model.module_list

        # ---- the plan (model/plan.py): shapes, activation / gradient buffers (same concat / slice structure), blocks, who writes first
        convs = {i: self._conv_attrs(mods[i]) for i, d in enumerate(defs) if d['type'] == 'convolutional'}
        # requires_grad is the engine's only selector of what trains (as for autograd), read now: Darknet.train_engine() keys its cache by
        # the pattern, so an engine never sees it change.  A frozen parameter is in no sink, no segment and gets no .grad; the plan drops
        # every backward launch, gradient buffer and workspace that only served frozen parameters (model/plan.py: `trainable`)
        self.tparams = [q for q in model.parameters() if q.requires_grad]
        self._tset = set(self.tparams)
        trainable = None if len(self.tparams) == sum(1 for _ in model.parameters()) else {i: self.block_trainable(mods[i]) for i in convs}
        tp = self._tplan = plan.plan_train(defs, convs, self.bs, self.H, self.W, cin=cin,
                                           yolos={i: (mods[i].na, model.nc + 6) for i, d in enumerate(defs) if d['type'] == 'yolo'},
                                           head_decode=sw.head_decode, trainable=trainable)

        def new_buf(c, h, w):
            return torch.empty((self.bs, h, w, c), dtype=torch.bfloat16, device=device)

        bufs = [new_buf(*b) for b in tp.buffers]
        tensors = {None: None}

        def tv(v):
            if v not in tensors:
                tensors[v] = bufs[v.buf][..., v.off:v.off + v.C]
            return tensors[v]

        self.x_nhwc = tv(tp.x)
        cmax = max(ops.cpad(max(c.out_channels, c.in_channels)) for c in (HipEngine._conv_of(mods[i]) for i in convs))
        self.ones = torch.ones(cmax, device=device)
        # where the kernels leave the per-channel sums of a frozen BatchNorm weight / bias, conv bias or slope: never flushed, never read
        self.dump = torch.zeros((3, cmax), device=device) if trainable is not None else None
        self.zeros = torch.zeros(cmax, device=device)
        self.stat_part = torch.zeros((tr.stat_rows(), 2, cmax), dtype=torch.float64, device=device)
        self.blocks = []                     # the ConvBlocks in layer order
        self.p = []
        self.static_grad = {}
        self.direct = False
        self.static_flat = None
        wgrad_ws, bn_ws = 0, 0
        self.plan = fwd = []    # (kind, layer, payload) in forward order: ConvBlock, AddRec / UpRec of tensors, YoloEntry
        self.packs = tr.WeightPackBatch(device)     # every conv's packed weights (forward + dgrad layouts): ONE launch per step
        for kind, i, rec in tp.forward:
            if kind == 'conv':
                blk = ConvBlock(rec, mods[i], tv, new_buf, device)
                self.packs.add(blk.conv.weight.detach(), blk.s, blk.cin_k, blk.packed, blk.packed_d)
                if blk.wgrad:
                    wgrad_ws = max(wgrad_ws, tr.wgrad_ws_bytes(blk.desc))
                if blk.bnbwd:
                    bn_ws = max(bn_ws, tr.bn_bwd_ws_bytes(blk.npix, blk.C))
                self.blocks.append(blk)
                fwd.append(('conv', i, blk))
            elif kind in ('add', 'up'):
                fwd.append((kind, i, type(rec)(*map(tv, rec))))
            elif kind == 'yolo':
                m = mods[i]
                c, h, w = tp.shapes[i]
                anchors = m.anchors.to(device=device, dtype=torch.float32).contiguous()
                pbuf = torch.empty((self.bs, m.na, h, w, model.nc + 6), dtype=torch.float32, device=device)
                # training returns the raw heads only (models.py:189-194): the decoded rows are not written -- the p-only form
                # of ryolo_yolo_decode needs the tiled kernel (no <= 96, na*no <= 1024); otherwise keep a scratch `io`
                io = None
                if model.nc + 6 > 96 or m.na * (model.nc + 6) > 1024:
                    io = torch.empty((self.bs, m.na * h * w, model.nc + 6), dtype=torch.float32, device=device)
                self.p.append(pbuf)
                hb = self.blocks[-1] if self.blocks and self.blocks[-1].i == i - 1 and self.blocks[-1].head_fused else None
                # a head nothing trainable feeds needs no gradient (the plan has none): the loss still writes one, into a scratch of the engine's
                head_g = tv(rec.head_g) if rec.head_g is not None else new_buf(c, h, w)
                fwd.append(('yolo', i, YoloEntry(tv(rec.head), head_g, m, anchors, pbuf, io, h, w, hb)))
        self.packs.finalize()
        self.nbt = [b.bn.num_batches_tracked for b in self.blocks if b.bn is not None]
        self.yolos = [pl for kind, _, pl in fwd if kind == 'yolo']
        # (head activation, head gradient) NHWC bf16 pairs in the order of self.p: the fused loss writes the gradients directly
        self.head_pairs = [(pl.head, pl.head_g) for pl in self.yolos]
        self.fused_nhwc = False
        self.head_g_ready = False
        # The head convs' bias gradients out of the fused loss's dense pass (csrc/loss.hip: rows of sums of the head gradient it stores,
        # added in the order of the pass they replace, so the gradients keep their bits): the backward then only
        # finalises the rows instead of re-reading the whole head gradient (bn_act_bwd's bias form).  Only for a head whose gradient the
        # NHWC loss kernel wrote (head_g_ready) and whose conv output feeds the yolo layer alone
        self.head_bias_fold = sw.head_bias_fold
        self.head_gscale = torch.ones(1, device=device)     # upstream gradient of the loss (written by the fused loss's backward)
        self.head_bias_ready = None      # per head: the rows the latest fused loss call wrote (None: none)
        self._bias_parts = self._bias_ws = None
        self._fold_now = (False,) * len(self.head_pairs)    # per head: this backward takes the bias gradient from the rows
        self._g_bwd_fold = None          # ... and what the captured backward graphs took
        readers = plan._readers(defs)
        for k, (hd, _) in enumerate(self.head_pairs):
            for b in self.blocks:
                i = b.i
                if (b.y is hd and b.bn is None and b.conv.bias is not None and b.conv.bias in self._tset and i + 1 < len(defs)
                        and defs[i + 1]['type'] == 'yolo' and readers[i] == [i + 1]):
                    b.head_k = k
        # (weight gradients on a second stream -- a parallel branch of the backward graphs -- were measured in rounds 2 and 5 and lost both
        #  times: 63.2 vs 62.6 ms, 50.07 vs 49.57 ms; wgrad_wide's two workgroups per CU fill the register file, nothing co-resides with it.
        #  The switch and its code were removed in round 6; profiles/r05_ab_log.txt keeps the numbers.)
        # round 5: the split-K reduces of a backward segment as ONE launch -- every layer keeps its partial tiles in its own workspace (3.2 GB
        # at bs 64 / 608^2) and the segment ends with ryolo_conv_wgrad_reduce_batch; bit-identical gradients.  False (the switch, or the
        # workspaces did not fit): one reduce launch behind every weight gradient, sharing the workspace _ws_w (rounds 2-4).
        self.batch_reduce = sw.batch_reduce
        self._wr_batches = {}
        self._ws_w_bytes = max(wgrad_ws, 256)
        self._ws_w = None               # allocated by _prepare_backward() when the per-layer path is in use
        self.ws_b = torch.empty(max(bn_ws, 256), dtype=torch.uint8, device=device)

        # ---- backward launch list: the forward entries reversed -- those whose output needs a gradient -- each with its static accumulate
        # flags (first contribution overwrites)
        entries = {(kind, i): pl for kind, i, pl in fwd}
        self.bplan = [(kind, i, entries[(kind, i)], flags) for kind, i, flags in tp.backward]

    @staticmethod
    def block_trainable(m):
        """(weight, affine, slope) of a `convolutional` block for plan_train's `trainable`: does Conv2d.weight train; the conv bias or a
        BatchNorm weight / bias; the activation's slope"""
        conv, bn = HipEngine._conv_of(m), HipEngine._bn_of(m)
        affine = [q for q in (conv.bias,) + ((bn.weight, bn.bias) if bn is not None else ()) if q is not None]
        slopes = [q for s_ in m if isinstance(s_, nn.PReLU) for q in s_.parameters()]
        return (bool(conv.weight.requires_grad), any(q.requires_grad for q in affine), any(q.requires_grad for q in slopes))

    @staticmethod
    def _conv_attrs(m):
        """what the planner reads of a `convolutional` block, from its modules; an activation without training kernels becomes the
        planner's refusal when the walk reaches the layer (Swish etc.: refuse instead of training them as linear)"""
        conv = HipEngine._conv_of(m)
        other = [type(s_).__name__ for s_ in m if not isinstance(s_, (nn.Conv2d, nn.BatchNorm2d, nn.PReLU, nn.LeakyReLU))
                 and type(s_).__name__ != 'Mish']
        return dict(cout=conv.out_channels, k=conv.kernel_size[0], s=conv.stride[0], pad=conv.padding[0],
                    bn=HipEngine._bn_of(m) is not None, act=None,
                    refuse="activation %s has no HIP training kernels (use model.backend = 'torch')" % other[0] if other else None)

    # ------------------------------------------------------------------ parameter gradients
    # The backward kernels ACCUMULATE (+=) into fp32 buffers with STABLE addresses (hipGraph replays write to the same
    # pointers every step).  Two sinks:
    #   own     engine-owned flat buffer, zeroed at the start of every backward and added to param.grad after the replay
    #           (param.grad may be None, a fresh tensor, anything the user does to it);
    #   direct  a data-parallel reducer is attached (dist.GradientAllReducer: param.grad IS a view of a flat bucket the
    #           reducer owns): the kernels accumulate straight into those views -- no per-step memset of a second 250-MB
    #           buffer and no 750-MB add pass.  The views' addresses are checked before every backward; if the user
    #           replaced a param.grad (e.g. zero_grad(set_to_none=True)) it is RE-BOUND to its bucket view -- zeroed when it
    #           was None, the replacement's values copied in otherwise (_check_direct_sink, _flush_param_grads): the sink,
    #           the captured graphs and the reducer's buckets stay as they are, and the all-reduce still sends this gradient.
    def _build_grad_sink(self):
        plist = self.tparams
        views = getattr(self.model, '_dp_grad_views', None)
        ok = views is not None
        if ok:
            for q in plist:
                v = views.get(q)
                if (v is None or v.dtype != torch.float32 or not v.is_contiguous() or v.device != q.device or v.shape != q.shape
                        or q.grad is None or q.grad.data_ptr() != v.data_ptr()):
                    ok = False
                    break
        self.direct = bool(ok)
        if ok:
            self.static_flat = None
            self.static_grad = {q: views[q] for q in plist}          # (holds the buckets' storage alive for the graphs)
        else:
            self.static_flat = torch.zeros(sum(q.numel() for q in plist), dtype=torch.float32, device=self.device)
            off = 0
            for q in plist:
                self.static_grad[q] = self.static_flat[off:off + q.numel()].view_as(q)
                off += q.numel()

    def _reset_grad_sink(self):
        """Forget the sink and every graph that holds its addresses (a reducer was attached / param.grad was replaced)."""
        self.static_grad, self.static_flat, self.direct = {}, None, False
        self._segs, self.g_bwd = None, None
        self._wr_batches = {}            # the batched reduces hold the sink's addresses

    def _check_direct_sink(self):
        """A reducer is attached and param.grad must BE the reducer's bucket view: its hooks all-reduce the buckets, so a gradient
        that lives anywhere else would be stepped on un-averaged (ranks diverge silently).  When the user replaced a param.grad --
        optimizer.zero_grad() sets it to None by default -- the view is put back: None means "zeroed" (the view is cleared), another
        tensor's values are copied in.  The sink, the graphs and the buckets stay as they are."""
        if not self.direct:
            return
        rebound = 0
        for q, v in self.static_grad.items():
            g = q.grad
            if g is None:
                v.zero_()
            elif g.data_ptr() != v.data_ptr():
                v.copy_(g)
            else:
                continue
            q.grad = v
            rebound += 1
        if rebound and not self._warned_rebind:
            self._warned_rebind = True
            import warnings
            warnings.warn("TrainEngine: %d param.grad tensors had been replaced (zero_grad(set_to_none=True)?) while a GradientAllReducer "
                          "owns them; they were re-bound to the reducer's buckets.  Use reducer.zero_grad() to clear gradients." % rebound)

    def _grad_of(self, p, row=0):
        if p not in self._tset:
            return self.dump[row]            # frozen: the kernel's sums go nowhere (row: BatchNorm weight 0, bias 1, slope 2)
        g = self.static_grad.get(p)
        if g is None:
            self._build_grad_sink()
            g = self.static_grad[p]
        return g

    def _flush_param_grads(self, params=None):
        """Add the engine's gradient buffers of `params` (default: all) into param.grad (own sink only: the direct sink IS
        param.grad), then run the parameters' post-accumulate-grad hooks (a data-parallel reducer launches a bucket's
        all-reduce from them)."""
        add_to, add_from = [], []
        plist = list(self.static_grad.keys()) if params is None else params
        if not self.direct:
            views = getattr(self.model, '_dp_grad_views', None) or {}
            for p in plist:
                g = self.static_grad[p]
                v = views.get(p)
                if v is not None and (p.grad is None or p.grad.data_ptr() != v.data_ptr()):
                    # a reducer owns this gradient: it must land in the bucket view the all-reduce sends (see _check_direct_sink)
                    if p.grad is None:
                        v.zero_()
                    else:
                        v.copy_(p.grad)
                    p.grad = v
                if p.grad is None:
                    p.grad = g.clone()
                else:
                    add_to.append(p.grad)
                    add_from.append(g)
            if add_to:
                torch._foreach_add_(add_to, add_from)
        for p in plist:
            hooks = getattr(p, '_post_accumulate_grad_hooks', None)
            if hooks:
                for hk in list(hooks.values()):
                    hk(p)

    def head_bias_parts(self, arc=0):
        """Per head the [rows, cpad] fp32 scratch the fused loss's dense pass writes its bias-gradient rows to (None where the fold is
        not served: another arc, more than 512 channels, a head conv without bias or with other readers), or None when the fold is
        switched off.  Allocated once per engine: the loss and the backward graphs hold these addresses."""
        if not self.head_bias_fold or arc != 0:
            return None
        if self._bias_parts is None:
            by_head = {b.head_k: b for b in self.blocks if b.head_k is not None}
            parts, ws = [], 256
            for k, q in enumerate(self.p):
                rows = tr.yolo_loss_bias_rows(q, arc) if k in by_head else 0
                parts.append(torch.empty((rows, ops.cpad(by_head[k].C)), dtype=torch.float32, device=self.device) if rows > 0 else None)
                if rows > 0:
                    ws = max(ws, tr.head_bias_ws_bytes(by_head[k].npix, by_head[k].C))
            self._bias_parts = parts
            self._bias_ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        return self._bias_parts if any(q is not None for q in self._bias_parts) else None

    def head_grad_buffers(self):
        """the fp32 head-gradient buffers (shaped like self.p) the loss writes and backward() converts: created on first use"""
        if self.static_pg is None:
            self.static_pg = [torch.zeros_like(p) for p in self.p]
        return self.static_pg

    def _prepare_backward(self):
        """Everything the backward launch list needs and a forward-only caller never did, allocated OUTSIDE any stream capture: the head
        gradients, the gradient sink, the folded-reduce plan and its scratch, layer 0's workspace for the path the plan chose, the job
        tables of the batched split-K reduce with the layers' own workspaces -- or, on the per-layer path (the switch, or those
        workspaces did not fit), the one shared workspace.  Idempotent: backward() calls it every step.  Returns the segments."""
        self.head_grad_buffers()
        if self.tparams:
            self._grad_of(self.tparams[0])               # make sure the gradient sink exists
        segs = self._segments()
        if self.batch_reduce:
            self._ensure_reduce_batches(segs)
        self._plan_reduce_fusion()
        if not self.batch_reduce and self._ws_w is None and any(kind == 'conv' and pl.has_wgrad for kind, _, pl, _ in self.bplan):
            self._ws_w = torch.empty(self._ws_w_bytes, dtype=torch.uint8, device=self.device)
        for b in self.blocks:
            if b.recompute and b.bnbwd and b.ws0 is None:
                b.ws0 = tr.conv0_bn_bwd_wgrad_ws(self.device) if b.one_pass else tr.conv0_bn_bwd_ws(self.device)
        if self.g_bwd is None:
            self.g_bwd = [None] * len(segs)
            self._g_bwd_fold = None
        return segs

    def _ensure_reduce_batches(self, segs):
        """One job table per backward segment for ryolo_conv_wgrad_reduce_batch: built OUTSIDE any stream capture (the table is uploaded
        from the host) and once per gradient sink (it holds the sink's addresses and the layers' own partial-tile workspaces).
        The per-layer workspaces add up to 3.2 GB at bs 64 / 608^2; when they do not fit, the engine falls back to the shared workspace
        and one reduce launch per layer and says so in `reduce_fallback` (bench.py prints it in launch_mode)."""
        try:
            self._build_reduce_batches(segs)
        except torch.cuda.OutOfMemoryError as e:
            for b in self.blocks:
                b.ws_w = None
            self._wr_batches = {}
            torch.cuda.empty_cache()
            self.batch_reduce = False
            self.reduce_fallback = "per-layer split-K reduces on one shared workspace (the per-layer workspaces did not fit: %s)" % str(e)[:120]
            self.g_bwd = None                 # graphs captured for the batched path (none yet on the first backward) are not reusable

    def _build_reduce_batches(self, segs):
        for lo, hi, _ in segs:
            if (lo, hi) in self._wr_batches:
                continue
            blks = [pl for kind, i, pl, flags in self.bplan[lo:hi] if kind == 'conv' and pl.has_wgrad]
            wb = None
            if blks:
                wb = tr.WgradReduceBatch(self.device)
                for b in blks:
                    if b.ws_w is None:
                        b.ws_w = torch.empty(max(tr.wgrad_ws_bytes(b.desc), 256), dtype=torch.uint8, device=self.device)
                    wb.add(b.desc, b.conv.in_channels, b.ws_w, self._grad_of(b.conv.weight), True)
                wb.finalize()
            self._wr_batches[(lo, hi)] = wb

    def _segments(self):
        """Cut the backward launch list where a data-parallel bucket (model._dp_buckets, lists of parameters, set by
        dist.GradientAllReducer) has received its last gradient, so the bucket's all-reduce over xGMI runs under the
        remaining backward kernels.  Returns [(lo, hi, params)], one entry when there is no reducer."""
        if self._segs is not None:
            return self._segs
        pos = {}
        for k, (kind, i, pl, flags) in enumerate(self.bplan):
            if kind == 'conv':
                for q in list(pl.conv.parameters()) + (list(pl.bn.parameters()) if pl.bn is not None else []) + (
                        list(pl.act.parameters()) if pl.act is not None else []):
                    if q in self._tset:
                        pos[q] = k
        cuts = set()
        for bucket in getattr(self.model, '_dp_buckets', None) or []:
            ks = [pos[q] for q in bucket if q in pos]
            if ks:
                cuts.add(max(ks) + 1)
        cuts.add(len(self.bplan))
        segs, lo = [], 0
        for hi in sorted(cuts):
            if hi > lo:
                segs.append((lo, hi, [q for q, k in pos.items() if lo <= k < hi]))
                lo = hi
        self._segs = segs
        return segs

    def forward(self, x):
        dev = self.device
        nhwc = isinstance(x, NHWC8Batch)
        if not nhwc:
            x = x.float().contiguous()
        with torch.cuda.device(dev), torch.no_grad():
            # the input converter runs OUTSIDE the graph, reading the caller's tensor where it lies: the graph starts at the
            # engine's own NHWC buffer, so no 283-MB staging copy of the batch into a graph-owned tensor
            if nhwc:        # already the input layout (model/nhwc_batch.py): a device-to-device copy, or nothing when it IS the buffer
                x.copy_into(self.x_nhwc)
            else:
                n, c, h, w = x.shape
                _lib.check(_lib.lib().ryolo_nchw_f32_to_nhwc_bf16(x.data_ptr(), n, c, h, w, 8, self.x_nhwc.data_ptr(), _lib.stream_ptr(dev)),
                           "ryolo_nchw_f32_to_nhwc_bf16")
            # what YOLOLayer.forward would have set (model_utils.py:16-35): the loss reads ng / anchor_vec.  On every call, replays
            # included: an evaluation at another size in between has changed the grids
            for yl in self.yolos:
                if (yl.module.nx, yl.module.ny) != (yl.nx, yl.ny):
                    create_grids(yl.module, (self.H, self.W), (yl.nx, yl.ny), dev)
            # two eager steps before the capture: every kernel's first launch (the library raises its LDS limit there), torch's own lazy
            # initialisation and the warm-up of the loss graph (model/loss_static.py)
            if not self.use_graph or self.steps < 2 or self.force_eager:
                self._forward_launch()
            else:
                if self.g_fwd is None:
                    self.g_fwd = self._capture(self._forward_launch)
                if self.g_fwd is not None:
                    self.g_fwd.replay()
        return [p for p in self.p]

    def _capture(self, launch):
        """One hipGraph of `launch()`.  If the capture fails -- e.g. a runtime that refuses stream capture while a multi-rank RCCL
        communicator has work in flight -- the engine falls back to eager launches for the rest of its life (slower, never wrong),
        runs `launch()` eagerly for this step and returns None; `graph_fallback` says why (bench.py prints it)."""
        dev = self.device
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):   # RCCL's watchdog thread must not void the capture
                launch()
            return g
        except Exception as e:      # noqa: BLE001  (whatever the runtime raises: the step must still run)
            self.use_graph = False
            self.graph_fallback = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")
            import warnings
            warnings.warn("TrainEngine: hipGraph capture failed (%s); continuing with eager launches" % self.graph_fallback)
            try:
                torch.cuda.synchronize(dev)
            except Exception:       # noqa: BLE001  (a sticky capture error surfaces here once; the stream is usable afterwards)
                pass
            launch()
            return None

    def _forward_launch(self):
        """the forward launch list (captured into g_fwd): launches and in-place tensor operations only"""
        dev = self.device
        L = _lib.lib()
        if self.nbt:
            torch._foreach_add_(self.nbt, 1)            # one launch for the 72 counters nn.BatchNorm2d would bump
        self.packs.run()
        for kind, i, pl in self.plan:
            if kind == 'conv':
                b = pl
                bn = b.bn
                if bn is not None:
                    part = tr.conv_fwd_stats(b.desc, b.xin, b.packed, self.ones, self.zeros, b.z, part=self.stat_part,
                                             clear=False)          # bn_finalize leaves the scratch zeroed (z None: sums only)
                    tr.bn_finalize(part, b.C, b.npix, bn.weight.detach(), bn.bias.detach(), eps=bn.eps, momentum=bn.momentum,
                                   running_mean=bn.running_mean, running_var=bn.running_var, out=b.stats)
                    if b.recompute:
                        tr.conv0_bn_act_fwd(b.desc, b.xin, b.packed, b.stats[2], b.stats[3], b.actcode, b.slope, b.y)
                    else:
                        tr.bn_act_fwd(b.z, b.stats[2], b.stats[3], b.actcode, b.slope, b.y, residual=b.res)
                elif b.head_fused is None:                 # (a fused head runs at its yolo entry, the next one)
                    tr.conv_fwd_plain(b.desc, b.xin, b.packed, self.ones, b.bias_now(self.zeros), b.z)
            elif kind == 'add':
                nn_, hh, ww, cc = pl.y.shape
                _lib.check(L.ryolo_add_nhwc(pl.a.data_ptr(), pl.a.stride(2), pl.b.data_ptr(), pl.b.stride(2), pl.y.data_ptr(), pl.y.stride(2),
                                            nn_ * hh * ww, cc, _lib.stream_ptr(dev)), "ryolo_add_nhwc")
            elif kind == 'up':
                nn_, hh, ww, cc = pl.x.shape
                _lib.check(L.ryolo_upsample_nhwc(pl.x.data_ptr(), pl.x.stride(2), pl.y.data_ptr(), pl.y.stride(2), nn_, hh, ww, cc, 2,
                                                 _lib.stream_ptr(dev)), "ryolo_upsample_nhwc")
            elif kind == 'yolo':
                hb, m = pl.fused_block, pl.module
                if hb is not None:
                    # the head conv, the raw p rows and the head tensor's store as one launch (csrc/conv_pw.hip MODE 5): the head is
                    # not written by one kernel and re-read by the next
                    tr.conv_head_decode_store(hb.head_fused, hb.xin, hb.packed, self.ones, hb.bias_now(self.zeros), pl.head, pl.p)
                else:
                    stride = float(max(self.H, self.W)) / float(max(pl.ny, pl.nx))
                    _lib.check(L.ryolo_yolo_decode(pl.head.data_ptr(), pl.head.stride(2), self.bs, pl.ny, pl.nx, m.na, self.model.nc + 6,
                                                   pl.anchors.data_ptr(), stride, 1.0, 0, pl.io.data_ptr() if pl.io is not None else None,
                                                   m.na * pl.ny * pl.nx, 0, pl.p.data_ptr(), _lib.stream_ptr(dev)), "ryolo_yolo_decode")

    # ------------------------------------------------------------------ backward
    def backward(self, pgrads):
        dev = self.device
        with torch.cuda.device(dev), torch.no_grad():
            segs = self._prepare_backward()
            ready, bias_ready = self.head_g_ready, self.head_bias_ready
            self.head_g_ready, self.head_bias_ready = False, None
            fold = [False] * len(self.static_pg)
            for k, (buf, g) in enumerate(zip(self.static_pg, pgrads)):
                if g is not None and ready and g.data_ptr() == buf.data_ptr():
                    fold[k] = bias_ready is not None and bias_ready[k] is not None     # ... and the rows of its bias gradient
                    continue                                  # the NHWC loss kernel already wrote this head's gradient
                if g is None:
                    buf.zero_()
                elif g.data_ptr() != buf.data_ptr():
                    buf.copy_(g)
                tr.pgrad_to_nhwc(buf, self.yolos[k].head_g)   # fp32 [bs,na,ny,nx,no] -> the head conv's NHWC bf16 gradient
                if self.fused_nhwc and g is not None:
                    buf.zero_()                               # keep the fused loss's scratch invariant (all zero)
            self._check_direct_sink()
            self._fold_now = tuple(fold)
            eager = not self.use_graph or self.steps < 2 or self.force_eager
            if not eager:
                # the graphs hold ONE source of the head bias gradients (the loss's rows or the pass over the head gradient); a step whose
                # head gradients arrive the other way (e.g. the eager loss mirror after fused steps) launches eagerly
                if self._g_bwd_fold is None:
                    self._g_bwd_fold = self._fold_now
                eager = self._g_bwd_fold != self._fold_now
            for k, (lo, hi, params) in enumerate(segs):
                if eager:
                    self._backward_launch(lo, hi)
                else:
                    if self.g_bwd[k] is None:
                        self.g_bwd[k] = self._capture(lambda lo=lo, hi=hi: self._backward_launch(lo, hi))
                    if self.g_bwd[k] is not None:
                        self.g_bwd[k].replay()
                self._flush_param_grads(params)
            self.steps += 1

    def _backward_launch(self, lo=0, hi=None):
        """entries lo..hi of the backward launch list (one segment, captured into g_bwd[k]) after _prepare_backward(): launches and
        in-place tensor operations only"""
        if lo == 0 and self.static_flat is not None:
            self.static_flat.zero_()
        if lo == 0 and self.dump is not None:
            self.dump.zero_()
        hook = self.backward_hook

        def entry(kind, i, pl, flags):
            if kind == 'yolo':
                pass                                          # converted (or written by the fused loss) before the segments run
            elif kind == 'conv':
                b = pl
                conv, bn = b.conv, b.bn
                res_first, in_first = flags
                dy = b.dy
                if b.res_g is not None and not b.res_alias:   # fused shortcut: the skip branch receives dy unchanged
                    self._passthrough(dy, b.res_g, res_first)
                if not b.bnbwd:
                    return                                    # only the skip source needed dy
                if bn is not None:
                    dsl = self._grad_of(b.act.weight, 2) if isinstance(b.act, nn.PReLU) else None
                    if b.one_pass:
                        # layer 0: BatchNorm / activation backward AND the weight gradient in one pass over dy (csrc/conv0_bwd.hip), no dz
                        tr.conv0_bn_bwd_wgrad(b.desc, b.xin, b.packed, dy, b.stats, b.actcode, b.slope,
                                              self._grad_of(bn.weight, 0), self._grad_of(bn.bias, 1), dsl, self._grad_of(conv.weight),
                                              conv.in_channels, True, b.ws0)
                        return
                    elif b.recompute:
                        tr.conv0_bn_bwd(b.desc, b.xin, b.packed, dy, b.stats, b.actcode, b.slope, b.dz,
                                        self._grad_of(bn.weight, 0), self._grad_of(bn.bias, 1), dsl, b.ws0)
                    elif b.red_part is not None:              # the reduce pass ran inside the data gradient that produced dy
                        tr.bn_act_bwd_reduced(b.z, dy, b.stats, 1, b.slope, b.dz,
                                              self._grad_of(bn.weight, 0), self._grad_of(bn.bias, 1), dsl, b.red_part, self.ws_b)
                    else:
                        tr.bn_act_bwd(b.z, dy, b.stats, b.actcode, b.slope, b.dz,
                                      self._grad_of(bn.weight, 0), self._grad_of(bn.bias, 1), dsl, self.ws_b)
                elif conv.bias is not None and conv.bias in self._tset:
                    if b.head_k is not None and self._fold_now[b.head_k]:
                        # the loss's dense pass summed the head gradient while storing it: finalise its rows (x the upstream gradient)
                        tr.head_bias_finalize(self._bias_parts[b.head_k], b.npix, b.C, self.head_gscale, self._grad_of(conv.bias), self._bias_ws)
                    else:
                        tr.bn_act_bwd(b.z, dy, None, 0, None, None, None, self._grad_of(conv.bias), None, self.ws_b)
                if not b.wgrad:
                    pass                                      # a frozen Conv2d.weight: no weight gradient at all
                elif self.batch_reduce:
                    # partial tiles only, into the layer's own workspace; the segment's reduces run as one launch below
                    tr.conv_wgrad_partials(b.desc, b.xin, b.dz, conv.in_channels, self._grad_of(conv.weight), True, b.ws_w)
                else:
                    tr.conv_wgrad(b.desc, b.xin, b.dz, conv.in_channels, self._grad_of(conv.weight), True, self._ws_w)
                if b.dgrad:
                    y = b.red_for
                    if y is not None:     # 1x1 data gradient + the reduce pass of the block whose output this conv consumed
                        tr.conv_dgrad_bnreduce(b.desc, b.dz, b.packed_d, self.ones, self.zeros, b.xin_g, not in_first,
                                               y.z, y.stats, y.slope, y.red_part)
                    else:
                        tr.conv_dgrad(b.desc, b.dz, b.packed_d, self.ones, self.zeros, b.xin_g, not in_first)
            elif kind == 'add':
                for g, is_first in zip((pl.a_g, pl.b_g), flags):
                    if g is not None:
                        self._passthrough(pl.dy, g, is_first)
            elif kind == 'up':
                if pl.x_g is not None:
                    tr.upsample2x_bwd(pl.dy, pl.x_g, not flags)

        for kind, i, pl, flags in self.bplan[lo:hi]:
            if hook is not None:
                hook('pre', kind, i, pl, flags)
            entry(kind, i, pl, flags)
            if hook is not None:
                hook('post', kind, i, pl, flags)
        if self.batch_reduce:
            wb = self._wr_batches[(lo, len(self.bplan) if hi is None else hi)]    # KeyError = partial tiles nobody would reduce
            if wb is not None:
                wb.run()                                      # the segment's split-K reduces, one launch

    def _plan_reduce_fusion(self):
        """Pairs (X, Y) of consecutive backward entries where X is a 1x1 conv whose data gradient writes the FINAL gradient of
        block Y's output (X consumed Y's output; in a residual chain X accumulates into the chain's running gradient, which
        is Y's dy) and Y is a BatchNorm + PReLU/leaky block: X's data gradient then also runs the reduce pass of Y's backward
        on the values it stores (ryolo_conv2d_dgrad_bnreduce), and Y only finalises and applies.  Planned once; the switch
        bn_reduce_fusion off: no pairs."""
        if self._red_planned:
            return
        self._red_planned = True
        if not self.switches.bn_reduce_fusion:
            return
        blk = {b.i: b for b in self.blocks}
        pairs = []
        for xr, yr, rows in plan.reduce_fusion_pairs(self._tplan):          # the static half: geometry, BatchNorm, the kernel's rows
            x, y = blk[xr['layer']], blk[yr['layer']]
            if y.actcode == 1:                                              # a BatchNorm block, not Mish, PReLU or LeakyReLU
                pairs.append((x, y, rows, x.xin_g.shape[3]))
        if not pairs:
            return
        # one scratch for all pairs: a pair's rows are consumed by the very next entry of the launch list
        part = torch.empty(max(rows * 3 * c for _, _, rows, c in pairs), dtype=torch.float32, device=self.device)
        for x, y, rows, c in pairs:
            x.red_for = y
            y.red_part = part[:rows * 3 * c].view(rows, 3, c)

    def _passthrough(self, src, dst, is_first):
        L = _lib.lib()
        n, h, w, c = dst.shape
        if is_first:
            _lib.check(L.ryolo_upsample_nhwc(src.data_ptr(), src.stride(2), dst.data_ptr(), dst.stride(2), n, h, w, c, 1,
                                             _lib.stream_ptr(self.device)), "ryolo_upsample_nhwc")
        else:
            _lib.check(L.ryolo_add_nhwc(src.data_ptr(), src.stride(2), dst.data_ptr(), dst.stride(2), dst.data_ptr(),
                                        dst.stride(2), n * h * w, c, _lib.stream_ptr(self.device)), "ryolo_add_nhwc")

    def __call__(self, x):
        anchor = self.tparams[0] if self.tparams else next(self.model.parameters())   # makes the Function part of the autograd graph
        return list(_Fn.apply(self, x, anchor))
