"""Dispatch census: every convolution launch the engines make over the accepted input space, and the kernel the library's
shape-driven dispatch picks for it.  A helper module of the suite (not a conftest): tests/test_dispatch_census.py (CPU tier) and
tests/test_dispatch_coverage_gpu.py (GPU tier) import it.

The plans come from the engines' own planner (rotate-yolov3_amd/model/plan.py), which needs no GPU; the cfg text stands in for the modules
(`_conv`), and test_dispatch_coverage_gpu.py::test_census_matches_the_engines checks that adapter against the engines field by field.

Call forms recorded per block:
  eval      ryolo_conv_kernel_choice(d, residual, 0) of the inference engine's single-conv launches
  pair      ryolo_conv_pair_supported: the fused stem pair of the inference engine (conv_stem.hip)
  head      ryolo_conv_head_decode_supported: a YOLO head conv + decode in one launch (conv_pw.hip)
  train     ryolo_conv_kernel_choice(d, 0, statistics) of the training forward (+ ryolo_conv0_recompute_supported)
  dgrad     ryolo_conv_dgrad_kernel_choice(d, with_bn_reduce), the flag as TrainEngine._plan_reduce_fusion sets it
  wgrad     ryolo_conv_wgrad_kernel_choice(d) and the split-K count (from ryolo_conv_wgrad_workspace_bytes)

Edge class = (form, kernel code, ksize, stride, edge bits); the bits are derived per kernel family from its launch code (each
helper below cites the lines it mirrors).  The device's CU count enters the persistent-grid bits: pass the real one on a GPU.
"""
import ctypes as C

import rotate_yolov3_amd  # noqa: F401  (installs the package under its importable name)
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import hip_ops as ops
from rotate_yolov3_amd.model import hip_train_ops as tr
from rotate_yolov3_amd.model import plan
from rotate_yolov3_amd.utils.parse_config import parse_model_cfg_text, yolo_mask

CONFIGS = (("darknet53", 1), ("darknet53", 2), ("darknet53", 15), ("tiny", 1), ("tiny", 80))
SQUARE = tuple((s, s) for s in range(320, 609, 32))
RECT = ((416, 640), (608, 352), (512, 384))          # (height, width)
SIZES = SQUARE + RECT
BATCHES = (1, 2, 4, 8, 16, 32, 64)

BK = 64          # conv_common.h:21 K elements per step
KP = 64          # wgrad.hip KP: pixels per weight-gradient K step
WGRAD_TAPS = 1000

DESC_FIELDS = [f for f, _ in ops.ConvDesc._fields_]


def desc_tuple(d):
    return tuple(round(getattr(d, f), 6) if f == "slope" else getattr(d, f) for f in DESC_FIELDS)


def mk_desc(t):
    return ops.ConvDesc(*t)


Refused = plan.Refused      # the engines refuse this configuration at plan time


def config_defs(kind, nc, H, W):
    text = make_cfg.darknet53(W, H, classes=nc) if kind == "darknet53" else make_cfg.tiny(W, H, classes=nc)
    defs = parse_model_cfg_text(text)
    assert defs[0]["type"] == "net"
    return defs[1:]


def _conv(d):
    k = int(d["size"])
    act = d.get("activation", "linear")
    return dict(cout=int(d["filters"]), k=k, s=int(d["stride"]), pad=(k - 1) // 2 if int(d.get("pad", 0)) else 0,
                bn=int(d["batch_normalize"]) != 0, act=ops.ACT_LEAKY if act == "leaky" else (ops.ACT_MISH if act == "mish" else ops.ACT_LINEAR),
                slope=0.1 if act == "leaky" else 0.0)


def _convs(defs):
    return {i: _conv(d) for i, d in enumerate(defs) if d["type"] == "convolutional"}


def _yolos(defs):
    return {i: (len(yolo_mask(d)), int(d["classes"]) + 6) for i, d in enumerate(defs) if d["type"] == "yolo"}


def _L():
    return _lib.lib()


def _choice(t, residual, stats):
    return _L().ryolo_conv_kernel_choice(C.byref(mk_desc(t)), 1 if residual else 0, 1 if stats else 0)


# ------------------------------------------------------------------------------------------------ the engines' conv launches
def eval_blocks(defs, H, W, N):
    """the conv launches of HipEngine's plan: [dict(form, layer, name, desc(s), ...)]"""
    recs = []
    for op in plan.plan_eval(defs, _convs(defs), _yolos(defs), N, H, W).ops:
        if op["kind"] == "conv":
            t = op["desc"]
            code = _choice(t, op["res"] is not None, False)
            recs.append(dict(form="eval", layer=op["layer"], desc=t, residual=op["res"] is not None, code=code,
                             name=ops.kernel_name_of(code, t[5], t[6], t[3]), out_off=op["out"].off, res_layer=op["res_layer"]))
        elif op["kind"] == "pair":
            recs.append(dict(form="pair", layer=op["layer"], descs=op["descs"], shortcut=op["shortcut"], code=1, name=op["name"]))
        elif op["kind"] == "head":
            recs.append(dict(form="head", layer=op["layer"], desc=op["desc"], na=op["na"], no=op["no"], code=1, name=op["name"]))
    return recs


def _has_wgrad(b):
    """every block but the one whose whole backward is one pass (layer 0: ryolo_conv0_bn_bwd_wgrad)"""
    return not (b["bn"] and b["recompute"] and b["one_pass"])


def train_blocks(defs, H, W, N):
    """TrainEngine's plan + the folded BatchNorm reduce: per conv block its descriptor and the four call forms"""
    tp = plan.plan_train(defs, _convs(defs), N, H, W)
    # the engine's run-time half of the fold: Y is a BatchNorm + PReLU / leaky block
    bnred = set(x["layer"] for x, y, rows in plan.reduce_fusion_pairs(tp) if y["act"] == ops.ACT_LEAKY)
    recs = []
    L = _L()
    for b in tp.blocks:
        dt = b["desc"]
        d = mk_desc(dt)
        code = L.ryolo_conv_kernel_choice(C.byref(d), 0, 1 if b["bn"] else 0)
        recs.append(dict(form="train", layer=b["layer"], desc=dt, code=code, stats=b["bn"], recompute=b["recompute"],
                         name=ops.kernel_name_of(code, dt[5], dt[6], dt[3])))
        if b["xin_g"] is not None:
            red = b["layer"] in bnred
            code = L.ryolo_conv_dgrad_kernel_choice(C.byref(d), 1 if red else 0)
            recs.append(dict(form="dgrad", layer=b["layer"], desc=dt, code=code, bnred=red,
                             name=ops.kernel_name_of(code, dt[5], 1, dt[4])))
        if _has_wgrad(b):
            code = L.ryolo_conv_wgrad_kernel_choice(C.byref(d))
            recs.append(dict(form="wgrad", layer=b["layer"], desc=dt, code=code, cin_real=3 if b["layer"] == 0 else dt[3], splits=wgrad_splits(dt, code)))
    return recs


# ------------------------------------------------------------------------------------------------ edge bits
def _out_hw(t):
    N, H, W, Cin, Cout, k, s, pad = t[:8]
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def _grid_bits(T, grid):
    """(underfull, ragged last round) of a persistent grid of `grid` workgroups walking T tiles"""
    return T < grid, T > grid and T % grid != 0


def _idle_wgs(code, M, Cout, cus):
    """conv_mp.hip:657 / conv_mq.hip:713-714: a tile list shorter than the persistent grid shrinks the grid to round8(T) workgroups; when
    T % 8 != 0 the surplus workgroups of the last XCD chunk exit at once"""
    if code not in (1, 2, 3, 9, 10):
        return False
    bm, bn = {1: (256, 256), 2: (192, 256), 3: (128, 256), 9: (128, 128), 10: (64, 128)}[code]
    T = -(-M // bm) * -(-Cout // bn)
    cap = (cus & ~7) if code in (1, 2) else 2 * (cus & ~7)
    return T < cap and T % 8 != 0


def _gemm_bits(code, M, Cout, ks, cus, stats, res, os_, force, kpad):
    """tile bits of the implicit-GEMM families for one launch of M pixels x Cout channels"""
    if code in (1, 2):          # conv_mp.hip:655-657 persistent grid of CUs & ~7; BM 256 / 192, BN 256 (MP_BN)
        bm, bn = (256 if code == 1 else 192), 256
        T = -(-M // bm) * -(-Cout // bn)
        return (M % bm != 0, Cout % bn != 0) + _grid_bits(T, cus & ~7)
    if code == 3:               # conv_mq.hip:706-714 mq_grid_for: 2 x (CUs & ~7) workgroups; 128 x 256 tiles
        T = -(-M // 128) * -(-Cout // 256)
        return (M % 128 != 0, Cout % 256 != 0) + _grid_bits(T, 2 * (cus & ~7))
    if code in (9, 10):         # conv_mq.hip 128-channel tiles (128 / 64 pixels)
        bm = 128 if code == 9 else 64
        T = -(-M // bm) * -(-Cout // 128)
        return (M % bm != 0, Cout % 128 != 0) + _grid_bits(T, 2 * (cus & ~7))
    if code >= 16:              # conv_common.h IGEMM_TILES; conv.hip conv_igemm_plan()'s persistent grid (conv_common.h persist_grid())
        bm, bn, waves, nst = {1: (128, 128, 8, 2), 2: (256, 64, 4, 2), 3: (256, 32, 4, 2), 4: (256, 128, 8, 3), 6: (128, 128, 8, 2),
                              7: (128, 128, 4, 2)}[code - 16]
        T = -(-M // bm) * -(-Cout // bn)
        grid = (2 * cus) & ~7
        # conv_dispatch.hip conv_plan(): the 1x1 128 x 128 pick leaves the persistent layout to the 4-wave tile; its short-K 3x3 rule forces the persistent grid
        no_persist = code == 17 and ks == 1
        persist_ok = os_ == 1 and (not stats or (waves == 4 and not res))
        persistent = False
        if nst == 2 and bm * bn <= (bm + bn) * BK and persist_ok and not no_persist and (ks == 1 or force):
            persistent = (T > grid) if force else (2 * T >= 5 * grid)
        under, ragged = _grid_bits(T, grid) if persistent else (False, False)
        return (M % bm != 0, Cout % bn != 0, under, ragged)
    raise KeyError(code)


def _pw_bits(M, Cout, Cin, cus, decode_nb=None, bnred=False):
    """conv_pw.hip:586-627 pw_pick: channel blocks of ncb, row blocks of pf * 16 pixels, grid = wgpc * (CUs & ~7) split over the blocks
    (bnred: the configurations of the data gradient that carries the folded BatchNorm reduce, conv_pw.hip:606-613)"""
    kt = Cin // 64
    c = cus & ~7
    if decode_nb is not None:
        ncb, pf, wgpc = (128 if kt == 16 else 256), 4, 1
        NB = decode_nb
    else:
        if kt == 4 and Cout <= 128 and not bnred:
            ncb, pf, wgpc = 128, 8, 2
        elif kt == 6 and Cout <= 128 and not bnred:
            ncb, pf, wgpc = 128, 4, 2
        elif kt == 2 and Cout % 256 == 0:
            ncb, pf, wgpc = 256, 4, 1
        elif kt in (4, 8):
            ncb, pf, wgpc = (128 if bnred else 256), 4, 1
        elif kt in (12, 16) and not bnred:
            ncb, pf, wgpc = 128, 4, 1
        else:
            raise ValueError("conv_pw serves no configuration for K %d, C_out %d (bnred %s)" % (Cin, Cout, bnred))
        NB = -(-Cout // ncb)
    grid = wgpc * c
    mb = -(-M // (pf * 16))
    per_block = grid // max(NB, 1)
    return (M % (pf * 16) != 0, Cout % ncb != 0) + _grid_bits(mb, per_block)


def _spatial_bits(Ho, Wo, N, th, tw, grid):
    """the halo / stem kernels: tiles of th x tw output pixels on a persistent grid (conv_stem.hip:973-978, 1136-1140, 1146-1151, 1115-1122)"""
    nt = N * -(-Ho // th) * -(-Wo // tw)
    return (Wo % tw != 0, Ho % th != 0) + _grid_bits(nt, grid)


def wgrad_reduce_kind(S, Cout, cin_real, ks):
    """wgrad.hip wgrad_plan (reduce_kind): the split-K reduce a layer takes -- 0 one element per thread, 1 four split quarters per workgroup
    (S >= 8), 2 the transposing 3x3 kernel (few splits, >= 2^20 weights)"""
    total = Cout * cin_real * ks * ks
    if S < 8 and ks == 3 and cin_real % 64 == 0 and total >= (1 << 20):
        return 2
    return 1 if S >= 8 else 0


def wgrad_splits(t, code):
    ws = _L().ryolo_conv_wgrad_workspace_bytes(C.byref(mk_desc(t)))
    N, H, W, Cin, Cout, k = t[:6]
    kpad = -(-(k * k * Cin) // 64) * 64
    per = (Cout * kpad * 4) if code > WGRAD_TAPS else (-(-Cout // 128) * 128 * kpad * 4)
    assert ws % per == 0, (t, ws, per)
    return ws // per


# ------------------------------------------------------------------------------------------------ the weight gradient's host decisions
WGRAD_TILE_VARIANTS = (0x1000, 0x2000, 0x2000 | 0x4000, 3 << 16)     # never the per-tap kernels; the square tile; the transposed tile; three splits
WGRAD_JOB_FIELDS = ("S", "Cout", "Cin_real", "Cin_k", "ks", "Kpad", "Cout_pad", "kind", "wide", "block_end")
_DUMMY = 4096            # a 16-byte aligned, non-null address: ryolo_conv_wgrad_reduce_job_fill stores it, nothing dereferences it


def wgrad_plan_record(t, cin_real):
    """(kernel code, workspace bytes, the job fields ryolo_conv_wgrad_reduce_job_fill writes) of one weight gradient"""
    L, d, job = _L(), mk_desc(t), tr.WgradReduceJob()
    L.ryolo_conv_wgrad_reduce_job_fill(C.byref(job), C.byref(d), cin_real, _DUMMY, _DUMMY, 0)
    return (L.ryolo_conv_wgrad_kernel_choice(C.byref(d)), L.ryolo_conv_wgrad_workspace_bytes(C.byref(d))) + tuple(getattr(job, f) for f in WGRAD_JOB_FIELDS)


def wgrad_plan_groups(configs=CONFIGS, sizes=SIZES, batches=BATCHES):
    """{"config/classes/HxW": sorted [descriptor..., cin_real, record...] rows}: every distinct weight gradient of the training engine over
    the census's input space, and the bs-64 608^2 ones again under each of WGRAD_TILE_VARIANTS"""
    ti = DESC_FIELDS.index("tile")
    groups = {}
    for kind, nc in configs:
        if kind != "darknet53":          # (the training engine's model)
            continue
        for (H, W) in sizes:
            defs = config_defs(kind, nc, H, W)
            keys = set()
            for N in batches:
                for b in plan.plan_train(defs, _convs(defs), N, H, W).blocks:
                    if not _has_wgrad(b):
                        continue
                    t, c = tuple(b["desc"]), 3 if b["layer"] == 0 else b["desc"][3]
                    keys.add((t, c))
                    if (H, W, N) == (608, 608, 64):
                        keys.update((t[:ti] + (v,) + t[ti + 1:], c) for v in WGRAD_TILE_VARIANTS)
            groups["%s/%d/%dx%d" % (kind, nc, H, W)] = sorted(list(t) + [c] + list(wgrad_plan_record(t, c)) for t, c in keys)
    return groups


def wgrad_plan_hashes(groups=None):
    """one sha256 per group of wgrad_plan_groups(): tests/golden/wgrad_plan.json holds the parent library's"""
    import hashlib
    import json
    groups = wgrad_plan_groups() if groups is None else groups
    return {k: hashlib.sha256(json.dumps(rows).encode()).hexdigest() for k, rows in groups.items()}


# ------------------------------------------------------------------------------------------------ the convolutions' host decisions
CONV_PLAN_PICKS = tuple(range(1, 18)) + (13 | (2 << 16),)            # every forced tile low byte; conv_pw.hip with a capped grid
CONV_PLAN_BITS = (0x100, 0x200, 0x800, 0x8000)                        # general path; no persistent grid; forced persistent grid; classic dgrad classes
CONV_PLAN_TUNES = (("RYOLO_CONV3X3", ("mp", "mq")), ("RYOLO_CONV1X1", ("igemm",)), ("RYOLO_BN_REDUCE_TILES", ("0", "2")),
                   ("RYOLO_STEM_DGRAD", ("0", "1", "2")))
CONV_PLAN_BASE = ((608, 608, 64, True), (608, 608, 1, True), (320, 320, 1, True), (608, 608, 32, False))     # (H, W, N, with the training plan)
PIXELS_MAX = 0x7fffffff - 512          # conv_dispatch.hip conv_shape(): the most pixels one launch indexes
SLICE_MAX = 1 << 31                    # bytes a tensor slice must stay below for the kernels' 31-bit buffer offsets


def _full(t):
    return desc_tuple(mk_desc(t))


def _with(t, **kw):
    return tuple(kw.get(f, v) for f, v in zip(DESC_FIELDS, t))


def dgrad_pixels(t):
    """pixels of the input gradient a data gradient of descriptor `t` writes"""
    return t[0] * t[1] * t[2]


def conv_plan_record(t):
    """every host decision the library's queries show for one conv descriptor: the forward kernel for (residual, statistics) in (0,0),
    (1,0), (0,1), (1,1); the data gradient's kernel plain and with the folded BatchNorm reduce, and the reduce's rows (None where the
    input gradient has more pixels than a launch indexes: those are refused, test_dispatch_census.py asserts that apart); whether the
    layer-0 recompute serves it"""
    L, d = _L(), mk_desc(t)
    fwd = [L.ryolo_conv_kernel_choice(C.byref(d), r, s) for s in (0, 1) for r in (0, 1)]
    if dgrad_pixels(t) > PIXELS_MAX:
        dg = [None, None, None]
    else:
        dg = [L.ryolo_conv_dgrad_kernel_choice(C.byref(d), 0), L.ryolo_conv_dgrad_kernel_choice(C.byref(d), 1), L.ryolo_conv2d_dgrad_bnreduce_rows(C.byref(d))]
    return fwd + dg + [L.ryolo_conv0_recompute_supported(C.byref(d))]


def _plan_points(defs, H, W, N, train):
    """(descriptors, fused ops) of the engines' plans at one point: the ops are ("pair", first, second, shortcut) / ("head", desc, na, no)"""
    descs, fused = set(), set()
    recs = eval_blocks(defs, H, W, N) + (train_blocks(defs, H, W, N) if train else [])
    for r in recs:
        if r["form"] == "pair":
            a, b = (_full(x) for x in r["descs"])
            descs.update((a, b))
            fused.add(("pair", a, b, 1 if r["shortcut"] else 0))
        elif r["form"] == "head":
            descs.add(_full(r["desc"]))
            fused.add(("head", _full(r["desc"]), r["na"], r["no"]))
        else:
            descs.add(_full(r["desc"]))
    return descs, fused


def _conv_plan_rows(descs, fused=()):
    L = _L()
    rows = [list(t) + conv_plan_record(t) for t in sorted(descs)]
    for op in sorted(fused):
        if op[0] == "pair":
            rows.append(["pair"] + list(op[1]) + list(op[2]) + [op[3], L.ryolo_conv_pair_supported(C.byref(mk_desc(op[1])), C.byref(mk_desc(op[2])), op[3])])
        else:
            rows.append(["head"] + list(op[1]) + [op[2], op[3], L.ryolo_conv_head_decode_supported(C.byref(mk_desc(op[1])), op[2], op[3])])
    return rows


def _raised_cstride(pixels, channels):
    """the smallest multiple of 8 at which `pixels` pixels of that stride, the last one `channels` wide, reach SLICE_MAX bytes"""
    cs = -(-(SLICE_MAX // 2 - channels) // (pixels - 1))
    return max(-(-cs // 8) * 8, -(-channels // 8) * 8)


def conv_guard_variants(t):
    """{name: descriptor}: `t` pushed over each size guard of the dispatch in turn"""
    N, H, W, Cin, Cout = t[:5]
    Ho, Wo = _out_hw(t)
    ups = t[DESC_FIELDS.index("upsample")]
    out = {"out_cstride": _with(t, out_cstride=_raised_cstride(N * Ho * Wo * ups * ups, Cout)),
           "in_cstride": _with(t, in_cstride=_raised_cstride(N * H * W, Cin)),
           "res_cstride": _with(t, res_cstride=_raised_cstride(N * Ho * Wo, Cout))}
    n = -(-(1 << 32) // (Ho * Wo * max(Ho, Wo)))               # M * max(Ho, Wo) >= 2^32: the multiply-high pixel split is no longer exact
    if n * Ho * Wo <= PIXELS_MAX:
        out["pixel_extent"] = _with(t, N=n)
    out["pixels"] = _with(t, N=PIXELS_MAX // (Ho * Wo) + 1)     # M > PIXELS_MAX
    return out


def conv_plan_groups(configs=CONFIGS, sizes=SIZES, batches=BATCHES):
    """{group: rows}: the host decisions of the forward convolution and the data gradient (conv_plan_record per descriptor; the fused
    pair / head ops of the plans with their *_supported answers)
      auto/config/classes/HxW   every distinct descriptor of eval_blocks and train_blocks over `batches`
      pick/v, bit/0x..          the base set (CONV_PLAN_BASE, darknet53 with one class) under each forced tile low byte / tile bit
      tune/NAME=value           the base set under each tuning switch (set through ryolo_set_tuning, cleared after the group)
      guard/name                the 608^2 bs-64 descriptors pushed over each size guard (conv_guard_variants)"""
    groups = {}
    for kind, nc in configs:
        for (H, W) in sizes:
            defs = config_defs(kind, nc, H, W)
            descs, fused = set(), set()
            for N in batches:
                try:
                    d, f = _plan_points(defs, H, W, N, kind == "darknet53")
                except Refused:
                    continue
                descs |= d
                fused |= f
            groups["auto/%s/%d/%dx%d" % (kind, nc, H, W)] = _conv_plan_rows(descs, fused)
    base, base_fused, bs64 = set(), set(), set()
    for (H, W, N, train) in CONV_PLAN_BASE:
        d, f = _plan_points(config_defs("darknet53", 1, H, W), H, W, N, train)
        base |= d
        base_fused |= f
        if N == 64:
            bs64 |= d
    ti = DESC_FIELDS.index("tile")
    for v in CONV_PLAN_PICKS:
        groups["pick/%d" % v] = _conv_plan_rows(set(_with(t, tile=v) for t in base))
    for b in CONV_PLAN_BITS:
        groups["bit/0x%x" % b] = _conv_plan_rows(set(_with(t, tile=t[ti] | b) for t in base))
    for name, values in CONV_PLAN_TUNES:
        for v in values:
            _lib.set_tuning(name, v)
            try:
                groups["tune/%s=%s" % (name, v)] = _conv_plan_rows(base, base_fused)
            finally:
                _lib.set_tuning(name, None)
    guards = {}
    for t in sorted(bs64):
        for name, g in conv_guard_variants(t).items():
            guards.setdefault(name, set()).add(g)
    for name, descs in guards.items():
        groups["guard/%s" % name] = _conv_plan_rows(descs)
    return groups


def conv_plan_hashes(groups=None):
    """one sha256 per group of conv_plan_groups(): tests/golden/conv_plan.json holds the parent library's"""
    import hashlib
    import json
    groups = conv_plan_groups() if groups is None else groups
    return {k: hashlib.sha256(json.dumps(rows).encode()).hexdigest() for k, rows in groups.items()}


def edge_bits(rec, cus):
    """named boolean edge bits of one census record"""
    form, code, t = rec["form"], rec["code"], rec.get("desc")
    if form == "pair":
        a, b = rec["descs"]
        Ho, Wo = _out_hw(b)
        # conv_stem.hip:28/33 (P<1>: 8 x 32 tiles), 573-600; grid 2 x CUs
        return dict(zip(("part_right", "part_bottom", "underfull", "ragged"), _spatial_bits(Ho, Wo, b[0], 8, 32, (2 * cus) & ~7)))
    N, H, W, Cin, Cout, k, s, pad, in_cs, out_cs = t[:10]
    Ho, Wo = _out_hw(t)
    names4 = ("part_m", "part_n", "underfull", "ragged")
    if form == "head":
        # conv_pw.hip:593-601: the decoded head: all anchors' channels in NB blocks, grid = CUs & ~7
        apb = (128 if Cin == 1024 else 256) // rec["no"]          # conv_pw.hip pw_decode_apb: whole anchors per channel block
        nb = -(-rec["na"] // apb)
        return dict(zip(names4, _pw_bits(N * H * W, Cout, Cin, cus, decode_nb=nb)))
    if form == "wgrad":
        M = N * Ho * Wo
        S = rec["splits"]
        if code > WGRAD_TAPS:
            # wgrad.hip wgrad_plan, the per-tap branch: K steps are 64-pixel row segments, `per` steps per split
            nsteps = N * Ho * -(-Wo // KP)
            per = -(-nsteps // S)
            return dict(ragged_split=nsteps % per != 0, part_row=Wo % KP != 0, short_row=Wo < KP, multi_split=S > 1,
                        reduce=wgrad_reduce_kind(S, Cout, rec["cin_real"], k))
        # wgrad.hip wgrad_plan, the general branch: chunk = ceil(M / S) rounded up to KP pixels; T the c_out tile (256 wide / 258-260 three-stage / square)
        chunk = -(-(-(-M // S)) // KP) * KP if S > 0 else M
        tco = 256 if code == 256 else (128 if code in (257, 258, 259) else (64 if code == 260 else code))
        return dict(ragged_split=M % chunk != 0, short_row=Wo < KP, part_k=M % KP != 0, part_co=Cout % tco != 0, multi_split=S > 1,
                    reduce=wgrad_reduce_kind(S, Cout, rec["cin_real"], k))
    if form in ("eval", "train"):
        stats = form == "train" and rec["stats"]
        res = form == "eval" and rec["residual"]
        if code == 4:            # conv.hip conv0_params(): 16-pixel groups, 32 groups per wave, 4 waves per block
            M = N * Ho * Wo
            return dict(part_group=M % 16 != 0, part_block=M % (16 * 32 * 4) != 0)
        if code == 8:            # conv_stem.hip:232 (8 x 64 tiles), 1136-1140 grid 4 x CUs
            return dict(zip(("part_right", "part_bottom", "underfull", "ragged"), _spatial_bits(Ho, Wo, N, 8, 64, (4 * cus) & ~7)))
        if code == 5:            # conv_stem.hip:28-33: 8 x 32 (stride 1) / 4 x 32 (stride 2)
            return dict(zip(("part_right", "part_bottom", "underfull", "ragged"),
                            _spatial_bits(Ho, Wo, N, 8 if s == 1 else 4, 32, (2 * cus) & ~7)))
        if code == 11:           # conv_stem.hip:741 (4 x 32 tiles), 973-978
            return dict(zip(("part_right", "part_bottom", "underfull", "ragged"), _spatial_bits(Ho, Wo, N, 4, 32, (2 * cus) & ~7)))
        M = N * Ho * Wo
        if code == 6:
            return dict(zip(names4, _pw_bits(M, Cout, Cin, cus)))
        kpad = -(-(k * k * Cin) // BK) * BK
        force = k == 3 and kpad // BK <= 9 and not (stats and (res or code == 18))    # conv_dispatch.hip conv_plan(): the short-K 3x3 rule
        bits = _gemm_bits(code, M, Cout, k, cus, stats, res, 1, force, kpad)
        return dict(zip(names4, bits), part_cstride=out_cs != Cout, idle_wgs=_idle_wgs(code, M, Cout, cus))
    if form == "dgrad":
        if code == 7:            # conv_stem.hip:1115-1122 (8 x 64 stride 2 / 4 x 32 stride 1 / 8 x 32 the 128-channel kernel)
            th, tw = (8, 64) if (Cin == 32 and s == 2) else ((4, 32) if Cin == 32 else (8, 32))
            return dict(zip(("part_right", "part_bottom", "underfull", "ragged"), _spatial_bits(H, W, N, th, tw, (2 * cus) & ~7)))
        # conv_dgrad.hip conv_dgrad(): stride 1 is one launch over the input pixels; stride 2 is two x-fused classes (pixel pairs, 2 C_in channels)
        # or four parity classes, each a launch with its own pixel count
        launches = []
        if s == 1:
            launches.append((N * H * W, Cin, 1))
        elif Cin <= 64 and Cin % 32 == 0 and W % 2 == 0 and in_cs == Cin:
            launches += [(N * ((H - a + 1) // 2) * (W // 2), 2 * Cin, 2) for a in (0, 1)]
        else:
            launches += [(N * ((H - a + 1) // 2) * ((W - b + 1) // 2), Cin, 2) for a in (0, 1) for b in (0, 1)]
        acc = [False] * 5
        for M, co, os_ in launches:
            if M <= 0:
                continue
            if code == 6:
                bits = _pw_bits(M, co, Cout, cus, bnred=rec["bnred"]) + (False,)
            else:
                kpad = -(-(k * k * Cout) // BK) * BK
                force = k == 3 and os_ == 1 and kpad // BK <= 9 and not rec["bnred"]
                bits = _gemm_bits(code, M, co, k, cus, False, False, os_, force, kpad) + (_idle_wgs(code, M, co, cus),)
            acc = [x or y for x, y in zip(acc, bits)]
        return dict(zip(names4 + ("idle_wgs",), acc), multi_launch=len(launches) > 1)
    raise KeyError(form)


def edge_class(rec, cus):
    t = rec.get("desc") or rec["descs"][1]
    bits = edge_bits(rec, cus)
    extra = ()
    if rec["form"] == "dgrad":
        extra = (("bnred", rec["bnred"]),)
    elif rec["form"] == "train":
        extra = (("stats", rec["stats"]), ("recompute", rec["recompute"]))
    elif rec["form"] == "eval":
        extra = (("residual", rec["residual"]), ("ups", t[13] == 2))
    return (rec["form"], rec["code"], t[5], t[6]) + extra + tuple(sorted(bits.items()))


def cost(rec):
    """M * K * C_out of the record's launch (the representative is the cheapest point of a class)"""
    t = rec.get("desc") or rec["descs"][1]
    Ho, Wo = _out_hw(t)
    return t[0] * Ho * Wo * t[5] * t[5] * t[3] * t[4]


def census(cus=256, configs=CONFIGS, sizes=SIZES, batches=BATCHES, refused=None):
    """{edge class: dict(count, rep)} over the input space; rep = the cheapest record reaching the class (ties: first seen).
    Points the engines refuse at plan time are skipped and listed in `refused` (a list, when given)."""
    classes = {}
    for kind, nc in configs:
        for (H, W) in sizes:
            defs = config_defs(kind, nc, H, W)
            for N in batches:
                try:
                    recs = eval_blocks(defs, H, W, N)
                except Refused as e:
                    if refused is not None:
                        refused.append(((kind, nc, H, W, N), str(e)))
                    continue
                if kind == "darknet53":
                    recs += train_blocks(defs, H, W, N)
                for r in recs:
                    r["point"] = (kind, nc, H, W, N)
                    key = edge_class(r, cus)
                    e = classes.get(key)
                    if e is None:
                        classes[key] = dict(count=1, rep=r)
                    else:
                        e["count"] += 1
                        if cost(r) < cost(e["rep"]):
                            e["rep"] = r
    return classes


def format_table(classes):
    rows = []
    for key in sorted(classes, key=lambda k: (k[0], k[1], k[2], k[3], str(k[4:]))):
        e = classes[key]
        r = e["rep"]
        t = r.get("desc") or r["descs"][1]
        bits = ",".join(k if v is True else "%s=%s" % (k, v) for k, v in key[4:] if v) or "-"
        rows.append("%-6s code %-4d k%d s%d  %-60s  n=%-5d rep %s layer %d  desc N%d %dx%d %d->%d cs %d/%d" % (
            key[0], key[1], key[2], key[3], bits, e["count"], r["point"], r["layer"], t[0], t[1], t[2], t[3], t[4], t[8], t[9]))
    return "\n".join(rows)
