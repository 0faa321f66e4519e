"""Layer planner -- the rules that turn a Darknet cfg into buffers and launches, once, on plain Python data.

No tensor is allocated and no device is touched here: HipEngine (model/engine.py) and TrainEngine (model/train_engine.py)
materialise a plan into tensors and closures, tests/dispatch_census.py walks the same plans without a GPU.  The only calls
into the library are its dry-run queries (pair / fused head / layer-0 recompute supported, rows of the folded BatchNorm reduce).

Input: the cfg `defs` (without the `net` block), batch and input size, `convs[i]` = dict(cout, k, s, pad, bn, act, slope) of
every `convolutional` layer (the engines read them from the modules: a fused model has lost its BatchNorm modules while its
defs still say batch_normalize=1; a `refuse` message in it is raised when the walk reaches that layer), `yolos[i]` = (na, no).
A layer that carries `weight_from` (`convolutional` or `d-convolutional`, the matrix cfgs) is described by shared_attrs(): `src`, the
layer whose weight it reads, `dil`, stride 1, no BatchNorm, linear -- what the reference computes for it (models.py:254-265).

A `View` is a channel slice of a buffer: (buffer id, channel offset, C, H, W, pixel stride); `buffers[id]` = (C, H, W) of the
NHWC bf16 allocation, buffer 0 is the 8-channel network input.  Two views are the same tensor exactly when they are equal.

The plan of both engines:
  * `shortcut` layers are folded into the producing conv as a residual operand, `upsample` x2 into its store (inference only);
  * sources of a multi-input `route` are written into channel slices ("homes") of the route's concat buffer by whoever
    produces them; single-input routes are aliases;
and, where the two differ, one explicit policy each: inference falls back to run-time copies / the small NHWC kernels and fuses
stem pairs and YOLO heads; training refuses what it has no kernels for, mirrors every activation buffer with a gradient buffer,
shares one gradient buffer along a residual chain and decides statically who writes a gradient view first.
"""
import ctypes as C
from collections import namedtuple

from .. import _lib
from .._lib import ACT_LINEAR, ConvDesc

View = namedtuple('View', 'buf off C H W cs')
EvalPlan = namedtuple('EvalPlan', 'shapes buffers x views ops')
CONV_TYPES = ('convolutional', 'd-convolutional')
TrainPlan = namedtuple('TrainPlan', 'shapes buffers x act grd forward blocks backward')
# the non-conv records of TrainPlan.forward: views here, the same types with tensors in TrainEngine.plan (x_g: gradient view of x, or None)
AddRec = namedtuple('AddRec', 'a b y a_g b_g dy')
UpRec = namedtuple('UpRec', 'x y x_g dy')
YoloRec = namedtuple('YoloRec', 'head head_g')


class Refused(RuntimeError):
    """the configuration is refused at plan time (as opposed to a bug in the planner)"""


def _abs(i, l):
    return l if l > 0 else i + l      # route/shortcut index convention of models.py:101-114 (0 is "relative")


def _sources(i, d):
    return [_abs(i, int(v)) for v in d['layers'].split(',')]


def shared_attrs(d):
    """convs[i] of a block with `weight_from`: F.conv2d(x, weight of layer src, padding, dilation) and nothing else -- stride 1 whatever
    the block says, no bias, BatchNorm or activation.  pad: 1 = "same" ((k-1)/2 * dilation per axis), 0 = none."""
    k = int(d['size'])
    dil = (1, 1)
    if d['type'] == 'd-convolutional':
        dil = tuple(int(t) for t in str(d['dilation']).strip().strip('()').split(','))
    pad = (k - 1) // 2 if int(d.get('pad', 0)) else 0
    return dict(cout=int(d['filters']), k=k, s=1, pad=pad, dil=dil, bn=False, act=ACT_LINEAR, slope=0.0, src=int(d['weight_from']),
                dilated=d['type'] == 'd-convolutional', refuse=None)


def _new(buffers, c, h, w):
    buffers.append((c, h, w))
    return View(len(buffers) - 1, 0, c, h, w, c)


def _slice(v, off, c):
    return View(v.buf, v.off + off, c, v.H, v.W, v.cs)


def _shapes(defs, convs, cin, H, W):
    """(C, H, W) per layer"""
    shp = []
    c, h, w = cin, H, W
    for i, d in enumerate(defs):
        t = d['type']
        if t in CONV_TYPES:
            cv = convs[i]
            dh, dw = cv.get('dil', (1, 1))
            c = cv['cout']
            h = (h + 2 * cv['pad'] * dh - dh * (cv['k'] - 1) - 1) // cv['s'] + 1
            w = (w + 2 * cv['pad'] * dw - dw * (cv['k'] - 1) - 1) // cv['s'] + 1
        elif t == 'maxpool':
            k, s = int(d['size']), int(d['stride'])
            if not (k == 2 and s == 1):
                p = (k - 1) // 2
                h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        elif t == 'upsample':
            s = int(d['stride'])
            h, w = h * s, w * s
        elif t == 'route':
            ls = _sources(i, d)
            c = sum(shp[l][0] for l in ls)
            h, w = shp[ls[0]][1], shp[ls[0]][2]
        shp.append((c, h, w))
    return shp


def _readers(defs):
    """who reads what (decides which epilogue fusions are legal)"""
    readers = [[] for _ in defs]
    for i, d in enumerate(defs):
        if d['type'] == 'route':
            for l in _sources(i, d):
                readers[l].append(i)
        else:
            if i > 0:
                readers[i - 1].append(i)
            if d['type'] == 'shortcut':
                readers[_abs(i, int(d['from']))].append(i)
    return readers


def _routes(defs, shp):
    """alias: single-input route -> its source; concat: multi-input route -> [(source with aliases resolved, channel offset)]"""
    alias, concat = {}, {}
    for i, d in enumerate(defs):
        if d['type'] != 'route':
            continue
        ls = _sources(i, d)
        if len(ls) == 1:
            alias[i] = ls[0]
            continue
        off = 0
        concat[i] = []
        for l in ls:
            src = l
            while src in alias:
                src = alias[src]
            concat[i].append((src, off))
            off += shp[l][0]
    return alias, concat


def _query(name, *descs_then_ints):
    args = [C.byref(ConvDesc(*a)) if isinstance(a, tuple) else a for a in descs_then_ints]
    return getattr(_lib.lib(), name)(*args)


def pair_descs(N, x, first, second, out_cs=None):
    """descriptor tuples of a fused stem pair reading view `x`: the tensor between the two convs is dense and never stored"""
    a = (N, x.H, x.W, x.C, first['cout'], first['k'], first['s'], first['pad'], x.cs, first['cout'], 0, first['act'], first['slope'], 1, 0)
    h1 = (x.H + 2 * first['pad'] - first['k']) // first['s'] + 1
    w1 = (x.W + 2 * first['pad'] - first['k']) // first['s'] + 1
    b = (N, h1, w1, first['cout'], second['cout'], second['k'], second['s'], second['pad'], first['cout'], out_cs or second['cout'], 0,
         second['act'], second['slope'], 1, 0)
    return a, b


# ------------------------------------------------------------------------------------------------ inference
def plan_eval(defs, convs, yolos, N, H, W, stem_pair=True, head_decode=True, cin=3):
    """EvalPlan(shapes, buffers, x, views, ops).  views[i]: the layer's output view, None where the tensor only lives in LDS (first
    layer of a fused pair) or is materialised on demand (fused head).  ops: dicts in launch order, kind =
      conv      layer, xin, out, res (view or None), res_layer, ups, desc
      pair      layer (the second conv), first, xin, out, shortcut, descs, name
      head      layer (the yolo layer), conv, xin, desc, na, no, name
      add       layer, a, b, out            upsample  layer, xin, out, stride        maxpool   layer, xin, out, size, stride
      copy      layer (the route), xin, out  decode    layer, xin                     se        layer, xin, out, C
      dconv     layer, xin, out, res, res_layer, dil, desc, name (csrc/conv_dil.hip: a dilated 3x3 with a shared weight)
      alias     layer, of: a shared-weight layer with the input view, source and geometry of the earlier layer `of` (and no residual) IS that
                layer's tensor -- nothing is launched (in the matrix cfgs the first 1x1 of every branch of a level)
    conv / dconv / head ops of a layer with `weight_from` carry src = the layer whose packed weight they read (scale 1, shift 0); the
    others have src None.  descriptors are tuples in ConvDesc field order."""
    n = len(defs)
    shp = _shapes(defs, convs, cin, H, W)
    for i, d in enumerate(defs):
        if d['type'] == 'route' and any(shp[l][1:] != shp[i][1:] for l in _sources(i, d)):
            raise Refused("route %d joins tensors of different spatial size (reorg is out of scope)" % i)
        if d['type'] == 'shortcut' and shp[_abs(i, int(d['from']))] != shp[i - 1]:
            raise Refused("shortcut %d adds tensors of different shape" % i)
    readers = _readers(defs)
    fused_into = {}     # follower layer (shortcut / upsample) -> conv layer that computes it
    conv_res, conv_ups = {}, set()
    for i, d in enumerate(defs):
        if i == 0 or defs[i - 1]['type'] not in CONV_TYPES or readers[i - 1] != [i] or (i - 1) in fused_into.values():
            continue
        if d['type'] == 'shortcut' and _abs(i, int(d['from'])) != i - 1:
            fused_into[i] = i - 1
            conv_res[i - 1] = _abs(i, int(d['from']))
        elif d['type'] == 'upsample' and int(d['stride']) == 2:
            fused_into[i] = i - 1
            conv_ups.add(i - 1)

    # homes: sources of multi-input routes live inside the route's concat buffer; the rest is copied at run time
    buffers = []
    x = _new(buffers, 8, H, W)
    views = [None] * n
    alias, concat = _routes(defs, shp)
    home, copies = {}, {}
    for i, srcs in concat.items():
        views[i] = _new(buffers, *shp[i])
        for src, off in srcs:
            if src not in home and defs[src]['type'] in CONV_TYPES + ('shortcut', 'upsample', 'maxpool', 'se') and src < i \
                    and shp[src][0] % 8 == 0 and off % 8 == 0:
                home[src] = _slice(views[i], off, shp[src][0])
            else:
                copies.setdefault(i, []).append((src, off))

    def view_for(i):
        return home[i] if i in home else _new(buffers, *shp[i])

    ops = []
    shared_seen = {}     # (input view, source layer, k, pad, dilation) -> the shared-weight layer that already computed it
    pending = None       # first layer of a fused stem pair, waiting for its successor
    pending_head = None  # last conv of a YOLO head, emitted together with its decode
    for i, d in enumerate(defs):
        t = d['type']
        if i in fused_into:
            views[i] = views[fused_into[i]]        # the conv already produced this layer's tensor
            continue
        if t in CONV_TYPES:
            cv = convs[i]
            if cv.get('refuse'):
                raise Refused(cv['refuse'])
            src = cv.get('src')                    # the layer whose weight a `weight_from` layer reads
            xin = x if i == 0 else views[i - 1]    # (None behind the first layer of a fused pair)
            cin_k = convs[pending['layer']]['cout'] if pending is not None else xin.C
            res = views[conv_res[i]] if i in conv_res else None
            ups = 2 if i in conv_ups else 1
            final = i + 1 if (i in conv_res or i in conv_ups) else i
            if cv['cout'] % 8 or cin_k % 8:
                raise Refused("conv %d: channel counts must be multiples of 8 for the HIP path" % i)
            if pending is not None:
                # second layer of a fused stem pair (csrc/conv_stem.hip): the first layer's tensor is computed into LDS, never stored
                first, pending = pending, None
                fc = convs[first['layer']]
                views[i] = out = view_for(final)
                ops.append(dict(kind='pair', layer=i, first=first['layer'], xin=first['xin'], out=out, shortcut=res is not None,
                                descs=pair_descs(N, first['xin'], fc, cv, out.cs),
                                name='conv_stem_pair<k%ds%d+k%ds%d%s>' % (fc['k'], fc['s'], cv['k'], cv['s'], '+res' if res is not None else '')))
                continue
            if src is not None:
                key = (xin, src, cv['k'], cv['pad'], cv['dil'])
                if res is None and ups == 1 and i not in home and key in shared_seen and not cv.get('no_alias'):
                    views[i] = views[shared_seen[key]]
                    ops.append(dict(kind='alias', layer=i, of=shared_seen[key]))
                    continue
            if cv.get('dilated'):
                # csrc/conv_dil.hip: 3x3, "same" padding, C_in a multiple of 64; the output never overlaps the input it reads around
                views[i] = out = view_for(final)
                desc = (N, xin.H, xin.W, xin.C, cv['cout'], cv['k'], 1, cv['pad'], xin.cs, out.cs, res.cs if res is not None else 0,
                        cv['act'], cv['slope'], 1, 0)
                if cv['pad'] == 0 or cv['k'] != 3:
                    raise Refused("d-convolutional %d: only size=3 with pad=1 (padding = dilation) is on the HIP path" % i)
                if xin.C % 64:
                    raise Refused("d-convolutional %d: %d input channels (the dilated kernel serves multiples of 64)" % (i, xin.C))
                if ups != 1:
                    raise Refused("d-convolutional %d: no fused upsample" % i)
                if out.buf == xin.buf and out.off < xin.off + xin.C and xin.off < out.off + out.C:
                    raise Refused("d-convolutional %d: its route home would make it write the tensor it reads (in place)" % i)
                if not _query('ryolo_conv2d_dilated_supported', desc, int(cv['dil'][0]), int(cv['dil'][1])):
                    raise Refused("d-convolutional %d: dilation %s / shape not served by ryolo_conv2d_dilated" % (i, (cv['dil'],)))
                if res is None and i not in home:
                    shared_seen.setdefault(key, i)
                ops.append(dict(kind='dconv', layer=i, xin=xin, out=out, res=res, res_layer=conv_res.get(i), dil=tuple(cv['dil']), desc=desc,
                                src=src, name='conv_dil<d%dx%d%s>' % (cv['dil'][0], cv['dil'][1], '+res' if res is not None else '')))
                continue
            alone = readers[i] == [i + 1] and i not in home and res is None and ups == 1
            if (head_decode and alone and not cv['bn'] and cv['act'] == ACT_LINEAR and cv['k'] == 1 and cv['s'] == 1 and
                    defs[i + 1]['type'] == 'yolo'):
                # a YOLO head: conv + decode in one launch (ryolo_conv_head_decode)
                na, no = yolos[i + 1]
                ht = (N, xin.H, xin.W, xin.C, cv['cout'], 1, 1, 0, xin.cs, cv['cout'], 0, ACT_LINEAR, 0.0, 1, 0)
                if _query('ryolo_conv_head_decode_supported', ht, int(na), int(no)):
                    pending_head = dict(kind='head', conv=i, xin=xin, desc=ht, na=na, no=no, name='conv_pw<k1,K%d>+decode' % xin.C, src=src)
                    continue
            if (stem_pair and alone and src is None and i not in conv_res and defs[i + 1]['type'] == 'convolutional' and (i + 1) not in conv_ups
                    and convs[i + 1]['bn']):
                nx = convs[i + 1]
                if nx.get('refuse'):
                    raise Refused(nx['refuse'])
                # a shortcut behind the pair must come from the first layer's own input (it is taken from the LDS image)
                if (i + 1) not in conv_res or views[conv_res[i + 1]] == xin:
                    a, b = pair_descs(N, xin, cv, nx)
                    if _query('ryolo_conv_pair_supported', a, b, 1 if (i + 1) in conv_res else 0):
                        pending = dict(layer=i, xin=xin)         # emitted together with layer i + 1
                        continue
            views[i] = out = view_for(final)
            desc = (N, xin.H, xin.W, xin.C, cv['cout'], cv['k'], cv['s'], cv['pad'], xin.cs, out.cs, res.cs if res is not None else 0,
                    cv['act'], cv['slope'], ups, 0)
            if src is not None and res is None and ups == 1 and i not in home:
                shared_seen.setdefault(key, i)
            ops.append(dict(kind='conv', layer=i, xin=xin, out=out, res=res, res_layer=conv_res.get(i), ups=ups, desc=desc, src=src))
        elif t == 'shortcut':
            views[i] = view_for(i)
            ops.append(dict(kind='add', layer=i, a=views[i - 1], b=views[_abs(i, int(d['from']))], out=views[i]))
        elif t == 'upsample':
            views[i] = view_for(i)
            ops.append(dict(kind='upsample', layer=i, xin=views[i - 1], out=views[i], stride=int(d['stride'])))
        elif t == 'maxpool':
            views[i] = view_for(i)
            ops.append(dict(kind='maxpool', layer=i, xin=views[i - 1], out=views[i], size=int(d['size']), stride=int(d['stride'])))
        elif t == 'se':
            # squeeze-and-excitation (ryolo_se_nhwc): never in place -- the residual unit behind it takes its skip from the se's input
            c = shp[i][0]
            if c % 8 or c < 16 or c > 2048:
                raise Refused("se %d: %d channels (the HIP path serves multiples of 8 from 16 to 2048)" % (i, c))
            views[i] = view_for(i)
            ops.append(dict(kind='se', layer=i, xin=views[i - 1], out=views[i], C=c))
        elif t == 'route':
            if i in alias:
                views[i] = views[alias[i]]
            for src, off in copies.get(i, ()):
                ops.append(dict(kind='copy', layer=i, xin=views[src], out=_slice(views[i], off, shp[src][0])))
        elif t == 'yolo':
            if pending_head is not None:
                ops.append(dict(pending_head, layer=i))
                pending_head = None                 # views[i] stays None: detect() materialises the head tensor on demand
            else:
                views[i] = views[i - 1]
                ops.append(dict(kind='decode', layer=i, xin=views[i]))
        elif t == 'reorg3d':
            views[i] = views[i - 1]
    return EvalPlan(shp, buffers, x, views, ops)


# ------------------------------------------------------------------------------------------------ training
def plan_train(defs, convs, N, H, W, conv0_recompute=True, conv0_one_pass=True, cin=3, yolos=None, head_decode=True, trainable=None):
    """TrainPlan(shapes, buffers, x, act, grd, forward, blocks, backward).  act[i] / grd[i]: activation / gradient view per layer
    (same concat / slice structure).  forward: (kind, layer, record) with kind =
      conv   a block: layer, desc, xin, xin_g (None for layer 0), y, dy, res, res_g, res_alias (the skip source's gradient IS dy),
             bn, act, shape (C, H, W of the conv output z), recompute / one_pass (layer 0 without stored z / dz); with BatchNorm
             z and dz are buffers of their own (unless recompute / one_pass), without they are y and dy;
             head_fused: None, or dict(desc, na, no) for a YOLO head whose conv, p rows and head-tensor store run as one launch
             (ryolo_conv_head_decode_store) -- the conditions of plan_eval's fused head: alone on its input, no BatchNorm, k1 s1, the
             library's own ryolo_conv_head_decode_supported (needs `yolos[i]` = (na, no); whether the block is linear is the engine's
             half: training reads the activation from the modules)
      add    AddRec        up  UpRec        yolo  YoloRec
    blocks: the conv records.  backward: (kind, layer, flags) in launch order (forward reversed); flags say which gradient views the
    entry is the FIRST to write (it overwrites, later ones accumulate): conv (res_g, xin_g), add (a_g, b_g), up x_g; yolo: head index.

    trainable: None (every parameter trains), or {layer: (weight, affine, slope)} -- which parameters of a `convolutional` block train:
    Conv2d.weight; the conv bias or a BatchNorm weight / bias; the activation's slope (a layer that is missing trains nothing).  A layer
    output NEEDS a gradient iff its block has a trainable parameter or one of its inputs needs one (conv input, shortcut source, route
    source, upsample input: what autograd's requires_grad would say).  A gradient view nobody needs is None -- in act / grd and in
    every record -- and has no buffer; `backward` keeps the entries whose output needs a gradient, with the FIRST flags computed over
    those.  A conv record says what its entry launches: `bnbwd` (the BatchNorm / activation / bias backward that makes dz: the conv
    branch needs a gradient; False only where a fused shortcut merely hands dy on to its skip source), `dgrad` (xin_g is needed) and
    `wgrad` (Conv2d.weight trains).  Layer 0's one-pass backward IS its weight gradient: with the stem's weight frozen the block takes
    the recompute backward with a dz of its own."""
    n = len(defs)
    if any(d['type'] == 'd-convolutional' or 'weight_from' in d for d in defs):
        # a sharer would train as a layer with weights of its own, BatchNorm and activation: a different network
        raise Refused("training path: weight_from / d-convolutional layers have no HIP training kernels (use model.backend = 'torch')")
    shp = _shapes(defs, convs, cin, H, W)
    for i, d in enumerate(defs):
        if d['type'] == 'upsample' and int(d['stride']) != 2:
            raise Refused("training path: only x2 upsampling")
        if d['type'] == 'se':
            # the planner below passes over block types it has no rule for: an se cfg would train a different network
            raise Refused("training path: se layers have no HIP training kernels (use model.backend = 'torch')")
        if d['type'] == 'maxpool':
            raise Refused("training path: maxpool graphs (yolov3-tiny) cannot train in the reference either "
                          "(model/loss.py:248 hard-codes three heads)")
    readers = _readers(defs)
    # which layer outputs need a gradient: one sweep in layer order (every input of a layer is an earlier layer)
    owns = [trainable is None or any(trainable.get(i, ())) for i in range(n)]
    need = [True] * n
    if trainable is not None:
        for i, d in enumerate(defs):
            t = d['type']
            if t == 'convolutional':
                need[i] = owns[i] or (i > 0 and need[i - 1])
            elif t == 'shortcut':
                need[i] = need[i - 1] or need[_abs(i, int(d['from']))]
            elif t == 'route':
                need[i] = any(need[l] for l in _sources(i, d))
            else:
                need[i] = i > 0 and need[i - 1]
    fused_into, conv_res = {}, {}
    for i, d in enumerate(defs):
        if d['type'] == 'shortcut' and i > 0 and defs[i - 1]['type'] == 'convolutional' and readers[i - 1] == [i] \
                and _abs(i, int(d['from'])) != i - 1 and convs[i - 1]['bn']:
            fused_into[i] = i - 1
            conv_res[i - 1] = _abs(i, int(d['from']))

    buffers = []
    x = _new(buffers, 8, H, W)

    def new_pair(c, h, w, g=True):
        return _new(buffers, c, h, w), (_new(buffers, c, h, w) if g else None)

    act, grd = [None] * n, [None] * n
    alias, concat = _routes(defs, shp)
    home = {}
    children = {}                        # concat gradient buffer -> the slices that live inside it
    for i, srcs in concat.items():
        act[i], grd[i] = new_pair(*shp[i], g=need[i])
        for src, off in srcs:
            if src in home or defs[src]['type'] not in ('convolutional', 'shortcut', 'upsample') or shp[src][0] % 8 or off % 8:
                raise Refused("training path: route %d needs a copy (unsupported graph)" % i)
            home[src] = (_slice(act[i], off, shp[src][0]), _slice(grd[i], off, shp[src][0]) if need[src] else None)
            if need[src]:
                children.setdefault(grd[i], []).append(home[src][1])

    def pair_for(i):
        return home[i] if i in home else new_pair(*shp[i], g=need[i])

    forward, blocks = [], []
    fin_g = {}                           # layer -> the gradient view of the block that computes it (a conv with its fused shortcut)
    for i, d in enumerate(defs):
        t = d['type']
        if i in fused_into:
            act[i], grd[i] = act[fused_into[i]], fin_g[i]    # (the conv's own grd is None where only the skip source needs dy)
            continue
        if t == 'convolutional':
            cv = convs[i]
            if cv.get('refuse'):
                raise Refused(cv['refuse'])
            xin, xin_g = (x, None) if i == 0 else (act[i - 1], grd[i - 1])
            final = i + 1 if i in conv_res else i
            # residual chain: the gradient of this block's output and of its skip source are the same tensor
            # (d(x + f(x)) passes dy to the skip branch unchanged) -- share ONE buffer instead of copying dy into the
            # source's gradient: the block reads dy before the branch's dgrad accumulates onto it (launch order)
            rg = grd[conv_res[i]] if (i in conv_res and final not in home and need[final]) else None
            res_alias = rg is not None and rg[2:5] == shp[final] and rg.cs == rg.C
            if res_alias:
                y, dy = _new(buffers, *shp[final]), rg            # (no gradient buffer of its own)
            else:
                y, dy = pair_for(final)
            fin_g[final] = dy
            act[i], grd[i] = y, (dy if need[i] else None)
            c, h, w = shp[i]
            desc = (N, xin.H, xin.W, xin.C, c, cv['k'], cv['s'], cv['pad'], xin.cs, c, 0, 0, 0.0, 1, 0)
            # layer 0 trains without its conv output: z0 (4 x the input, 27 MACs per value) is recomputed in the BatchNorm
            # passes instead of being stored and re-read (include/ryolo.h: ryolo_conv0_*); its one-pass backward never materialises dz
            recompute = bool(i == 0 and cv['bn'] and i not in conv_res and conv0_recompute
                             and _query('ryolo_conv0_recompute_supported', desc))
            wgrad = bool(need[i] and (trainable is None or trainable.get(i, (False,))[0]))
            head_fused = None
            if (head_decode and yolos is not None and i + 1 < n and defs[i + 1]['type'] == 'yolo' and readers[i] == [i + 1] and i not in home
                    and i not in conv_res and not cv['bn'] and cv['k'] == 1 and cv['s'] == 1 and c % 8 == 0):
                na, no = yolos[i + 1]
                ht = (N, xin.H, xin.W, xin.C, c, 1, 1, 0, xin.cs, c, 0, ACT_LINEAR, 0.0, 1, 0)
                if _query('ryolo_conv_head_decode_supported', ht, int(na), int(no)):
                    head_fused = dict(desc=ht, na=int(na), no=int(no))
            blk = dict(layer=i, desc=desc, xin=xin, xin_g=xin_g, y=y, dy=dy, res=act[conv_res[i]] if i in conv_res else None,
                       res_g=grd[conv_res[i]] if i in conv_res else None, res_alias=res_alias, bn=cv['bn'], act=cv['act'], shape=shp[i],
                       recompute=recompute, one_pass=bool(recompute and xin_g is None and conv0_one_pass and wgrad), head_fused=head_fused,
                       bnbwd=need[i], dgrad=bool(need[i] and xin_g is not None), wgrad=wgrad)
            blocks.append(blk)
            forward.append(('conv', i, blk))
        elif t == 'shortcut':
            a, b = i - 1, _abs(i, int(d['from']))
            act[i], grd[i] = pair_for(i)
            forward.append(('add', i, AddRec(act[a], act[b], act[i], grd[a], grd[b], grd[i])))
        elif t == 'upsample':
            act[i], grd[i] = pair_for(i)
            forward.append(('up', i, UpRec(act[i - 1], act[i], grd[i - 1], grd[i])))
        elif t == 'route':
            if i in alias:
                act[i], grd[i] = act[alias[i]], grd[alias[i]]
        elif t == 'yolo':
            act[i], grd[i] = act[i - 1], grd[i - 1]
            forward.append(('yolo', i, YoloRec(act[i], grd[i])))

    # static accumulate flags of the backward pass (reverse order; the first contribution to a gradient view overwrites it)
    init = set()

    def first(g):
        if g in init:
            return False
        init.add(g)
        init.update(children.get(g, ()))      # writing a whole concat gradient initialises its channel slices
        return True

    heads = [i for kind, i, _ in forward if kind == 'yolo']
    backward = []
    for kind, i, pl in reversed(forward):
        if not need[i + 1 if (kind == 'conv' and i in conv_res) else i]:
            continue                                              # nobody needs a gradient this entry could write
        if kind == 'yolo':
            first(pl.head_g)                                      # always the first (sole) writer of the head gradient
            backward.append((kind, i, heads.index(i)))
        elif kind == 'conv':
            res_first = first(pl['res_g']) if (pl['res_g'] is not None and not pl['res_alias']) else None
            backward.append((kind, i, (res_first, first(pl['xin_g']) if pl['dgrad'] else None)))
        elif kind == 'add':
            backward.append((kind, i, tuple(first(g) if g is not None else None for g in (pl.a_g, pl.b_g))))
        elif kind == 'up':
            backward.append((kind, i, first(pl.x_g) if pl.x_g is not None else None))
    return TrainPlan(shp, buffers, x, act, grd, forward, blocks, backward)


def reduce_fusion_pairs(tp):
    """The static half of the folded BatchNorm reduce: [(X, Y, rows)] block records of consecutive backward entries where X is a 1x1
    conv whose data gradient writes the FINAL gradient of block Y's output (X consumed Y's output; in a residual chain X accumulates
    into the chain's running gradient, which is Y's dy), that gradient is contiguous and Y has a stored-z BatchNorm.  Whether Y's
    activation lets X's data gradient carry the reduce (ryolo_conv2d_dgrad_bnreduce, `rows` partial sums) is the caller's half."""
    by = {b['layer']: b for b in tp.blocks}
    pairs = []
    runs = set((k, i) for k, i, _ in tp.backward)
    order = [(k, i) for k, i, _ in reversed(tp.forward)]      # neighbours in the WHOLE list: a frozen pattern keeps a subset of the pairs
    for (k0, i0), (k1, i1) in zip(order[:-1], order[1:]):
        if k0 != 'conv' or k1 != 'conv' or (k0, i0) not in runs or (k1, i1) not in runs:
            continue
        x, y = by[i0], by[i1]
        g, dy = x['xin_g'], y['dy']
        if not x['dgrad'] or not y['bnbwd'] or not y['bn'] or y['recompute'] or g != dy or dy[2:5] != y['shape'] or g.cs != g.C:
            continue
        rows = _query('ryolo_conv2d_dgrad_bnreduce_rows', x['desc'])
        if rows > 0:
            pairs.append((x, y, rows))
    return pairs
