"""HipEngine -- static layer plan of a Darknet cfg on the MI355X hot path.

Built once per (input shape, device) from `Darknet.module_defs` / `module_list` (the reference walks the cfg
dynamically on every forward, model/models.py:244-298).  The planning rules live in model/plan.py (tensor-free, shared with
TrainEngine and the dispatch census); this class allocates the plan's buffers, packs weights, folds BatchNorm and builds one closure
per launch.  The plan:

  * every tensor is NHWC bf16 resident in HBM; a `View` = (buffer, channel offset, C, H, W);
  * `shortcut` layers are folded into the producing conv's epilogue as a residual operand (models.py:281-282);
  * `upsample` layers are folded into the producing conv's epilogue as a 2x2 replicated store (models.py:93-94);
  * multi-input `route` layers own one concat buffer and their sources are WRITTEN INTO channel slices of it by
    whoever produces them (models.py:269-278: torch.cat copies); single-input routes are aliases;
  * BatchNorm (eval) is folded to fp32 scale/shift applied on the fp32 accumulator (utils/torch_utils.py:45-69),
    PReLU(1)/LeakyReLU become the epilogue's slope;
  * the three YOLO decodes write straight into one [bs, sum(na*ny*nx), no] tensor (the torch.cat of models.py:298).
  * a layer with `weight_from` (the "matrix" cfgs) is F.conv2d with its source layer's weight and nothing else (models.py:254-265): it
    launches with the source's packed image -- packed once -- and scale 1 / shift 0; `d-convolutional` ones run ryolo_conv2d_dilated
    (csrc/conv_dil.hip); a sharer that repeats an earlier sharer's computation aliases its tensor (RYOLO_SHARED_ALIAS=0: launches again).
  * `se` layers run ryolo_se_nhwc (csrc/se.hip: pool, gate, scale) into a buffer of their own: their input has a second reader.
Whatever cannot be folded falls back to the small NHWC kernels of csrc/yolo.hip (add / upsample / copy / maxpool).
All launches go to torch's current stream through the C ABI; after a warm-up the sequence can be replayed from a
hipGraph (`use_graph=True`).
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from .. import _lib
from . import hip_ops as ops
from . import plan
from .nhwc_batch import NHWC8Batch
from .plan import _abs  # noqa: F401  (the cfg's layer-index convention, for callers that walk module_defs themselves)


class HipEngine(object):
    def __init__(self, model, x_shape, device, use_graph=False, want_p=True):
        _lib.lib()   # fail loudly if the HIP library is missing
        self.device = device
        self.bs, cin, self.H, self.W = [int(v) for v in x_shape]
        if self.H % 32 or self.W % 32:
            raise RuntimeError("input height/width must be multiples of 32")
        self.want_p = want_p
        self.use_graph = use_graph
        self.graph = None
        self.graph_layers = None     # the layers without the input converter: what an NHWC8Batch replays
        defs = model.module_defs
        mods = model.module_list
        cf = float((model.hyp or {}).get('context_factor', 1.0))
        arc = model.arc
        self.arc_code = 0 if 'default' in arc else (1 if 'BCE' in arc else 2)
        yolos = self.yolo_idx(defs)
        self.no = (model.nc + 6) if yolos else 0

        # ---- the plan (model/plan.py): shapes, buffers, one view per layer, the launches.  RYOLO_STEM_PAIR=0 keeps one launch per layer
        # of the Darknet-53 stem (layers 0-1 and 2-4, ryolo_conv2d_bn_act_pair), RYOLO_HEAD_DECODE=0 keeps a YOLO head's conv + decode as
        # two launches (A/B timing, tests)
        no_alias = os.environ.get("RYOLO_SHARED_ALIAS", "1") == "0"
        pl = plan.plan_eval(defs, {i: (dict(plan.shared_attrs(d), no_alias=no_alias) if 'weight_from' in d else self._conv_attrs(mods[i]))
                                   for i, d in enumerate(defs) if d['type'] in plan.CONV_TYPES},
                            {i: (mods[i].na, self.no) for i in yolos}, self.bs, self.H, self.W,
                            stem_pair=os.environ.get("RYOLO_STEM_PAIR", "1") != "0",
                            head_decode=os.environ.get("RYOLO_HEAD_DECODE", "1") != "0", cin=cin)
        self.shapes = shp = pl.shapes
        bufs = [torch.empty((self.bs, h, w, c), dtype=torch.bfloat16, device=device) for (c, h, w) in pl.buffers]
        tensors = {None: None}

        def tv(v):
            if v not in tensors:
                tensors[v] = bufs[v.buf][..., v.off:v.off + v.C]
            return tensors[v]

        self.x_nhwc = tv(pl.x)
        self.views = [tv(v) for v in pl.views]

        # ---- ops
        self.ops = []
        self.decodes = []   # (op index, head view, ny, nx, na, anchors, stride, cf, row offset) per yolo layer
        self.op_info = []   # per op: kind / kernel name / algorithmic flops and bytes (bench + profiling)
        self.keep = []      # tensors the closures reference
        self.total_rows = sum(mods[i].na * shp[i][1] * shp[i][2] for i in yolos)
        self.io = torch.empty((self.bs, self.total_rows, self.no), dtype=torch.float32, device=device) if yolos else None
        self.p = []
        row_off = 0
        params = {}         # conv layer -> its packed weights / folded BatchNorm, in launch order

        def conv_params(i, cin_k, src=None):
            if src is not None:
                # a weight_from layer: the source's packed image (one copy serves the source's own launch and every sharer), no BatchNorm, no bias
                sp = conv_params(src, cin_k)
                if 'ones' not in sp:
                    cp = ops.cpad(sp['cout'])
                    sp['ones'], sp['zeros'] = torch.ones(cp, device=device), torch.zeros(cp, device=device)
                    self.keep += [sp['ones'], sp['zeros']]
                return dict(sp, scale=sp['ones'], shift=sp['zeros'])
            if i in params and params[i]['cin_pad'] == cin_k:
                return params[i]
            conv, bn = self._conv_of(mods[i]), self._bn_of(mods[i])
            packed = ops.pack_weights(conv.weight.detach().float(), cin_pad=cin_k)
            if bn is not None:
                scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
                shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
                if conv.bias is not None:
                    shift = shift + conv.bias.detach().float() * scale
            else:
                scale = torch.ones(conv.out_channels, device=device)
                shift = conv.bias.detach().float() if conv.bias is not None else torch.zeros(conv.out_channels, device=device)
            cp = ops.cpad(conv.out_channels)
            scale, shift = ops.pad_vec(scale, cp), ops.pad_vec(shift, cp)
            self.keep += [packed, scale, shift]
            params[i] = dict(packed=packed, scale=scale, shift=shift, cout=conv.out_channels, cin=conv.in_channels,
                             wnumel=conv.weight.numel(), k=conv.kernel_size[0], cin_pad=cin_k)
            return params[i]

        def flops(i, hw):
            pr = params[i] if isinstance(i, int) else i         # (a weight_from layer passes its source's record)
            return 2.0 * pr['k'] ** 2 * pr['cin'] * pr['cout'] * hw[1] * hw[2] * self.bs

        # one scratch for every se layer: the ops are serial on one stream
        se_bytes = max([_lib.lib().ryolo_se_workspace_bytes(self.bs, op['out'].H, op['out'].W, op['C']) for op in pl.ops if op['kind'] == 'se'] or [0])
        se_ws = torch.empty(se_bytes, dtype=torch.uint8, device=device) if se_bytes else None

        for op in pl.ops:
            kind, i = op['kind'], op['layer']
            xin, out = tv(op.get('xin')), tv(op.get('out'))
            info = dict(kind=kind, layer=i, name=kind + '_nhwc', flops=0.0)
            if kind == 'alias':
                continue                # this layer's tensor IS an earlier shared layer's (views[i] already says so): nothing to launch
            if kind == 'dconv':
                t = op['desc']
                cv, res = conv_params(i, t[3], op['src']), tv(op['res'])
                self.ops.append(self._mk_dconv(xin, cv, t[4], op['dil'], t[11], t[12], res, out))
                info.update(kind='conv', name=op['name'], flops=flops(cv, shp[i]),
                            bytes=2.0 * self.bs * (t[1] * t[2] * cv['cin'] + shp[i][1] * shp[i][2] * t[4] * (2 if res is not None else 1)) + 2.0 * cv['wnumel'])
            elif kind == 'conv':
                t = op['desc']
                cv, res, ups = conv_params(i, t[3], op.get('src')), tv(op['res']), op['ups']
                self.ops.append(self._mk_conv(xin, cv['packed'], cv['scale'], cv['shift'], t[4], t[5], t[6], t[7], t[11], t[12], res, out, ups))
                # the kernel the library's dispatch takes for this launch (csrc/conv_dispatch.hip conv_plan(): the plan the launch executes)
                info.update(name=ops.conv_kernel_name(*t[:8], in_cs=t[8], out_cs=t[9], res_cs=t[10], upsample=ups, residual=res is not None),
                            flops=flops(cv, shp[i]),
                            bytes=2.0 * self.bs * (t[1] * t[2] * cv['cin'] + shp[i][1] * shp[i][2] * t[4] * (ups * ups + (1 if res is not None else 0)))
                            + 2.0 * cv['wnumel'])
            elif kind == 'pair':
                # two conv layers in one launch (csrc/conv_stem.hip): the first layer's tensor is computed into LDS, never stored
                f, (a, b) = op['first'], op['descs']
                c1, c2 = conv_params(f, a[3]), conv_params(i, b[3])
                self.ops.append(self._mk_pair(a, b, xin, c1, c2, op['shortcut'], out))
                info.update(kind='conv', name=op['name'], flops=flops(f, shp[f]) + flops(i, shp[i]),
                            bytes=2.0 * self.bs * (a[1] * a[2] * c1['cin'] + shp[i][1] * shp[i][2] * b[4]) + 2.0 * (c1['wnumel'] + c2['wnumel']))
            elif kind in ('head', 'decode'):
                m = mods[i]
                c, h, w = shp[i]
                anchors = m.anchors.to(device=device, dtype=torch.float32).contiguous()
                stride = float(max(self.H, self.W)) / float(max(h, w))      # model_utils.py:19-20
                pbuf = torch.empty((self.bs, m.na, h, w, self.no), dtype=torch.float32, device=device) if want_p else None
                self.p.append(pbuf)
                self.keep.append(anchors)
                io_bytes = self.bs * m.na * h * w * self.no * (4.0 + (4.0 if want_p else 0.0))
                if kind == 'head':
                    # a YOLO head's conv + decode in one launch (ryolo_conv_head_decode); detect() materialises the head tensor on demand
                    hc = dict(conv_params(op['conv'], op['desc'][3], op.get('src')), xin=xin)
                    head = dict(t=None, conv=hc, shape=(self.bs, h, w, hc['cout']))
                    self.ops.append(self._mk_head_decode(op['desc'], hc, m.na, anchors, stride, cf, row_off, pbuf))
                    info.update(kind='conv', name='conv_pw<k1,K%d>+decode' % hc['cin'], flops=flops(hc, shp[i]),
                                bytes=2.0 * self.bs * h * w * hc['cin'] + 2.0 * hc['wnumel'] + io_bytes)
                else:
                    head = xin
                    self.ops.append(self._mk_decode(head, h, w, m.na, anchors, stride, cf, row_off, pbuf))
                    info.update(name='yolo_decode', bytes=2.0 * self.bs * m.na * h * w * self.no + io_bytes)
                self.decodes.append((len(self.ops) - 1, head, h, w, m.na, anchors, stride, cf, row_off))
                row_off += m.na * h * w
            elif kind == 'add':
                self.ops.append(self._mk_add(tv(op['a']), tv(op['b']), out))
                info.update(bytes=6.0 * out.numel())
            elif kind == 'se':
                # fp32 copies taken now: a later in-place edit of the parameters rebuilds the engine (Darknet._drop_stale_eval_engines)
                w1 = mods[i].fc[0].weight.detach().to(device=device, dtype=torch.float32).contiguous().clone()
                w2 = mods[i].fc[2].weight.detach().to(device=device, dtype=torch.float32).contiguous().clone()
                self.keep += [w1, w2, se_ws]
                self.ops.append(self._mk_se(xin, w1, w2, out, se_ws))
                info.update(bytes=3.0 * 2.0 * out.numel())
            elif kind == 'maxpool':
                self.ops.append(self._mk_maxpool(xin, out, op['size'], op['stride']))
                info.update(bytes=2.0 * (xin.numel() + out.numel()))
            else:                       # upsample; a route source that has no home in the concat buffer is copied as an upsample x1
                self.ops.append(self._mk_upsample(xin, out, op.get('stride', 1)))
                info.update(name='upsample_nhwc', bytes=4.0 * out.numel() if kind == 'copy' else 2.0 * (xin.numel() + out.numel()))
            self.op_info.append(info)

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def yolo_idx(defs):
        return [i for i, d in enumerate(defs) if d['type'] == 'yolo']

    @staticmethod
    def _conv_of(m):
        for s in m:
            if isinstance(s, nn.Conv2d):
                return s
        raise RuntimeError("convolutional block without Conv2d")

    @staticmethod
    def _bn_of(m):
        for s in m:
            if isinstance(s, nn.BatchNorm2d):
                return s
        return None

    @staticmethod
    def _act_of(m):
        for s in m:
            if isinstance(s, nn.PReLU):
                if s.weight.numel() != 1:
                    raise RuntimeError("per-channel PReLU is not on the HIP path")
                return ops.ACT_LEAKY, float(s.weight.detach().float().item())
            if isinstance(s, nn.LeakyReLU):
                return ops.ACT_LEAKY, float(s.negative_slope)
            if type(s).__name__ == 'Mish':
                return ops.ACT_MISH, 0.0
            if not isinstance(s, (nn.Conv2d, nn.BatchNorm2d)):
                # an activation (Swish, ...) the HIP conv epilogue does not implement must not silently run as linear
                raise RuntimeError("activation %s is not on the HIP path (use model.backend = 'torch')" % type(s).__name__)
        return ops.ACT_LINEAR, 0.0

    @classmethod
    def _conv_attrs(cls, m):
        """what the planner reads of a `convolutional` block, from its MODULES (a fused model has no BatchNorm left, whatever its cfg says);
        an activation off the HIP path becomes the planner's refusal when the walk reaches the layer"""
        conv = cls._conv_of(m)
        try:
            (act, slope), refuse = cls._act_of(m), None
        except RuntimeError as e:
            (act, slope), refuse = (ops.ACT_LINEAR, 0.0), str(e)
        return dict(cout=conv.out_channels, k=conv.kernel_size[0], s=conv.stride[0], pad=conv.padding[0], bn=cls._bn_of(m) is not None,
                    act=act, slope=slope, refuse=refuse)

    def _mk_head_decode(self, desc, hc, na, anchors, stride, cf, row_off, pbuf):
        d = ops.ConvDesc(*desc)

        def run():
            _lib.check(_lib.lib().ryolo_conv_head_decode(C.byref(d), hc['xin'].data_ptr(), hc['packed'].data_ptr(), hc['scale'].data_ptr(),
                                                         hc['shift'].data_ptr(), anchors.data_ptr(), na, self.no, stride, cf, self.arc_code,
                                                         self.io.data_ptr(), self.total_rows, row_off,
                                                         pbuf.data_ptr() if pbuf is not None else None, _lib.stream_ptr(self.device)),
                       "ryolo_conv_head_decode")
        return run

    def _head_tensor(self, lazy):
        """the head tensor of a fused head, for detect()'s decode + filter kernel: allocated and computed on demand"""
        hc = lazy['conv']
        if lazy['t'] is None:
            lazy['t'] = torch.empty(lazy['shape'], dtype=torch.bfloat16, device=self.device)
        ops.conv2d_bn_act(hc['xin'], hc['packed'], hc['scale'], hc['shift'], hc['cout'], 1, stride=1, pad=0, act=ops.ACT_LINEAR, out=lazy['t'])
        return lazy['t']

    def _mk_pair(self, a, b, xin, c1, c2, shortcut, out):
        a, b = ops.ConvDesc(*a), ops.ConvDesc(*b)

        def run():
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().ryolo_conv2d_bn_act_pair(C.byref(a), C.byref(b), xin.data_ptr(), c1['packed'].data_ptr(),
                                                               c1['scale'].data_ptr(), c1['shift'].data_ptr(), c2['packed'].data_ptr(),
                                                               c2['scale'].data_ptr(), c2['shift'].data_ptr(), 1 if shortcut else 0,
                                                               out.data_ptr(), _lib.stream_ptr(self.device)), "ryolo_conv2d_bn_act_pair")
        return run

    def _mk_conv(self, xin, packed, scale, shift, cout, k, s, pad, act, slope, res, out, ups):
        def run():
            ops.conv2d_bn_act(xin, packed, scale, shift, cout, k, stride=s, pad=pad, act=act, slope=slope, residual=res,
                              out=out, upsample=ups)
        return run

    def _mk_dconv(self, xin, cv, cout, dil, act, slope, res, out):
        def run():
            ops.conv2d_dilated(xin, cv['packed'], cv['scale'], cv['shift'], cout, dil, act=act, slope=slope, residual=res, out=out)
        return run

    def _mk_add(self, a, b, out):
        n, h, w, c = out.shape

        def run():
            _lib.check(_lib.lib().ryolo_add_nhwc(a.data_ptr(), a.stride(2), b.data_ptr(), b.stride(2), out.data_ptr(),
                                                 out.stride(2), n * h * w, c, _lib.stream_ptr(self.device)), "ryolo_add_nhwc")
        return run

    def _mk_se(self, xin, w1, w2, out, ws):
        def run():
            ops.se_nhwc(xin, w1, w2, out=out, workspace=ws)
        return run

    def _mk_upsample(self, xin, out, s):
        n, h, w, c = xin.shape

        def run():
            _lib.check(_lib.lib().ryolo_upsample_nhwc(xin.data_ptr(), xin.stride(2), out.data_ptr(), out.stride(2), n, h, w,
                                                      c, s, _lib.stream_ptr(self.device)), "ryolo_upsample_nhwc")
        return run

    def _mk_maxpool(self, xin, out, k, s):
        n, h, w, c = xin.shape

        def run():
            _lib.check(_lib.lib().ryolo_maxpool_nhwc(xin.data_ptr(), xin.stride(2), out.data_ptr(), out.stride(2), n, h, w,
                                                     c, k, s, _lib.stream_ptr(self.device)), "ryolo_maxpool_nhwc")
        return run

    def _mk_decode(self, head, ny, nx, na, anchors, stride, cf, row_off, pbuf):
        def run():
            _lib.check(_lib.lib().ryolo_yolo_decode(head.data_ptr(), head.stride(2), self.bs, ny, nx, na, self.no,
                                                    anchors.data_ptr(), stride, cf, self.arc_code, self.io.data_ptr(),
                                                    self.total_rows, row_off, pbuf.data_ptr() if pbuf is not None else None,
                                                    _lib.stream_ptr(self.device)), "ryolo_yolo_decode")
        return run

    # ------------------------------------------------------------------ run
    def _as_input(self, x):
        """an NHWC8Batch as it is (already the engine's input layout), anything else as a contiguous fp32 NCHW tensor"""
        if tuple(x.shape) != (self.bs, x.shape[1], self.H, self.W) or x.shape[1] > 8:
            raise RuntimeError("engine was planned for input %s" % ((self.bs, x.shape[1], self.H, self.W),))
        return x if isinstance(x, NHWC8Batch) else x.float().contiguous()

    def _launch_input(self, x):
        if isinstance(x, NHWC8Batch):       # no converter pass: a device-to-device copy, or nothing when the batch IS the input buffer
            x.copy_into(self.x_nhwc)
            return
        n, c, h, w = x.shape
        _lib.check(_lib.lib().ryolo_nchw_f32_to_nhwc_bf16(x.data_ptr(), n, c, h, w, 8, self.x_nhwc.data_ptr(),
                                                          _lib.stream_ptr(self.device)), "ryolo_nchw_f32_to_nhwc_bf16")

    def _launch_layers(self):
        for op in self.ops:
            op()

    def _launch_all(self, x):
        self._launch_input(x)
        self._launch_layers()

    def detect(self, x, conf_thres=0.5, nms_thres=0.5, capacity=1 << 18, nms_style='OR'):
        """forward + post-processing for inference: the yolo layers run the fused decode + confidence filter +
        compaction kernel (ryolo_yolo_decode_filter; the [bs, rows, no] `io` tensor is never written), the survivors go
        through ONE segmented rotated-NMS launch.  Returns what non_max_suppression(model(x)[0], conf_thres, nms_thres)
        returns: list[bs] of [k, 8] rows (x, y, w, h, a, score, class_conf, class) by descending score, or None.
        nms_style: 'OR' or 'MERGE' (utils/nms/nms.py), handed to the NMS step."""
        from ..utils.nms.nms import check_nms_style, nms_from_candidates
        check_nms_style(nms_style)
        x = self._as_input(x)
        L = _lib.lib()
        dev = self.device
        skip = set(d[0] for d in self.decodes)
        with torch.cuda.device(dev):
            while True:
                if getattr(self, '_cand_cap', 0) < capacity:
                    self._cand = torch.empty((capacity, 8), dtype=torch.float32, device=dev)
                    self._cand_row = torch.empty(capacity, dtype=torch.int64, device=dev)
                    self._cand_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
                    self._cand_cap = capacity
                self._cand_cnt.zero_()
                self._launch_input(x)
                for k, op in enumerate(self.ops):
                    if k not in skip:
                        op()
                for (_, head, ny, nx, na, anchors, stride, cf, row_off) in self.decodes:
                    if isinstance(head, dict):
                        head = self._head_tensor(head)
                    _lib.check(L.ryolo_yolo_decode_filter(head.data_ptr(), head.stride(2), self.bs, ny, nx, na, self.no,
                                                          anchors.data_ptr(), stride, cf, self.arc_code, float(conf_thres), 2.0,
                                                          self.total_rows, row_off, self._cand.data_ptr(),
                                                          self._cand_row.data_ptr(), self._cand_cnt.data_ptr(), self._cand_cap,
                                                          _lib.stream_ptr(dev)), "ryolo_yolo_decode_filter")
                m = int(self._cand_cnt.item())
                if m <= self._cand_cap:
                    break
                capacity = 2 * m                      # the candidate buffer overflowed: grow it and run again
            if m == 0:
                return [None] * self.bs
            rowid, o = self._cand_row[:m].sort()      # the reference's order: (image, row) ascending
            cand = self._cand[:m][o]
            return nms_from_candidates(torch.div(rowid, self.total_rows, rounding_mode='floor'), cand, self.bs, nms_thres,
                                       nc=self.no - 6, nms_style=nms_style)

    def __call__(self, x):
        x = self._as_input(x)
        with torch.cuda.device(self.device):
            if not self.use_graph:
                self._launch_all(x)
            elif isinstance(x, NHWC8Batch):
                # the batch goes into the input buffer in front of a graph of the layers alone (as in TrainEngine.forward); the graph of
                # the fp32 path below owns a static fp32 input and the converter, and stays as it is
                self._launch_input(x)
                if self.graph_layers is None:
                    self._launch_layers()                    # warm-up, as below
                    torch.cuda.synchronize(self.device)
                    self.graph_layers = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph_layers, capture_error_mode="thread_local"):
                        self._launch_layers()
                self.graph_layers.replay()
            else:
                if self.graph is None:
                    self.static_x = x.clone()
                    self._launch_all(self.static_x)          # warm-up: one-time attribute setup happens here
                    torch.cuda.synchronize(self.device)
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                        self._launch_all(self.static_x)
                self.static_x.copy_(x)
                self.graph.replay()
        return self.io, tuple(self.p)
