"""Float64 restatement of weighted-merge rotated NMS (include/ryolo.h: ryolo_rnms_merge_segmented) -- not a test module.

merge_loop is the reference's greedy loop (utils/nms/nms.py:71-127, nms_style == 'MERGE') written literally over the oracle's CPU
restatement of the NMS IoU (oracle.riou.riou_matrix): take the first box still alive, its members are the alive boxes whose IoU with it
exceeds the threshold plus the box itself, the kept box becomes their score-weighted mean, the members leave.  The one stated deviation
is the angle: a member's angle enters the mean as a_j - pi * rint((a_j - a_i) / pi), a_i the kept box's angle.

pipeline restates utils.nms.nms.nms_from_candidates(..., nms_style='MERGE') in numpy; clustered is the input generator the tests share."""
import numpy as np

from oracle import riou

PI = 3.14159265358979323846


def merge_loop(d, thr, iou=None):
    """d [n, >=6] fp32 rows (cx, cy, w, h, a, score), sorted by score descending.  -> dict of
    keep bool [n]; owner int64 [n] (itself for a kept row); merged float64 [n, 5] (zeros for rows not kept);
    size int64 [n]: members of a kept row's group; vmax float64 [n, 5]: the largest |field| among them, the angle after folding;
    folded: how many members' angles were moved by a multiple of pi."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    n = len(d)
    if iou is None:
        iou = riou.riou_matrix(d, d)
    t = np.float32(thr)
    alive = np.ones(n, dtype=bool)
    keep = np.zeros(n, dtype=bool)
    owner = np.arange(n, dtype=np.int64)
    merged = np.zeros((n, 5), dtype=np.float64)
    size = np.zeros(n, dtype=np.int64)
    vmax = np.zeros((n, 5), dtype=np.float64)
    folded = 0
    with np.errstate(invalid='ignore'):
        over = iou > t                                   # NaN compares false, inf true: as the kernel's `iou > thr`
    while alive.any():
        i = int(np.argmax(alive))                        # the first alive box: the highest score left
        mem = alive & over[i]
        mem[i] = True
        idx = np.nonzero(mem)[0]
        v = d[idx, :5].astype(np.float64)
        w = d[idx, 5].astype(np.float64)
        ai = np.float64(d[i, 4])
        turns = np.rint((v[:, 4] - ai) / PI)
        folded += int(np.count_nonzero(turns))
        v[:, 4] = v[:, 4] - PI * turns
        with np.errstate(all='ignore'):
            sw = w.sum()
            if np.isfinite(sw) and sw > 0:
                merged[i] = (w[:, None] * v).sum(0) / sw
            else:
                merged[i] = d[i, :5].astype(np.float64)
        keep[i] = True
        owner[idx] = i
        size[i] = len(idx)
        vmax[i] = np.abs(v).max(0)
        alive[idx] = False
    return dict(keep=keep, owner=owner, merged=merged, size=size, vmax=vmax, folded=folded)


def bound(ref):
    """per kept row and field: ulp32(ref) + 4 (m + 1) 2^-53 max_j |v_j| -- two fp64 evaluations of the same quotient in different
    summation orders differ by at most the second term, and rounding each to fp32 can then differ by one ulp"""
    with np.errstate(all='ignore'):
        ulp = np.spacing(np.abs(ref['merged'].astype(np.float32))).astype(np.float64)
    return ulp + 4.0 * (ref['size'][:, None] + 1) * 2.0 ** -53 * ref['vmax']


def segmented(d, offsets, thr):
    """merge_loop over the segments [offsets[s], offsets[s+1]) of d, owners as global rows: the outputs of ryolo_rnms_merge_segmented"""
    d = np.ascontiguousarray(d, dtype=np.float32)
    n = len(d)
    out = dict(keep=np.zeros(n, dtype=bool), owner=np.arange(n, dtype=np.int64), merged=np.zeros((n, 5)), size=np.zeros(n, dtype=np.int64),
               vmax=np.zeros((n, 5)), folded=0)
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        lo, hi = int(lo), int(hi)
        if hi <= lo:
            continue
        r = merge_loop(d[lo:hi], thr)
        for k in ('keep', 'merged', 'size', 'vmax'):
            out[k][lo:hi] = r[k]
        out['owner'][lo:hi] = r['owner'] + lo
        out['folded'] += r['folded']
    return out


def pipeline(img, cand, bs, thr, nc):
    """nms_from_candidates(img, cand, bs, thr, nc=nc, nms_style='MERGE') in numpy.  -> (rows, bounds): per image the [k, 8] float64 rows
    (columns 0..4 the float64 weighted means, 5..7 the candidates' own) by descending score, or None; and the [k, 5] bounds of columns 0..4"""
    cand = np.ascontiguousarray(cand, dtype=np.float32)
    img = np.asarray(img, dtype=np.int64)
    o1 = np.argsort(-cand[:, 5], kind='stable')
    seg = (img * nc + cand[:, 7].astype(np.int64))[o1]
    o2 = np.argsort(seg, kind='stable')
    order = o1[o2]
    seg = seg[o2]
    det = cand[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(seg))[0] + 1, [len(seg)]])
    ref = segmented(det[:, :6], starts, thr)
    keep = ref['keep']
    rows = np.concatenate([ref['merged'][keep], det[keep][:, 5:].astype(np.float64)], 1)
    bnd = bound(ref)[keep]
    dimg = img[order][keep]
    o3 = np.argsort(-rows[:, 5], kind='stable')
    o4 = np.argsort(dimg[o3], kind='stable')
    o = o3[o4]
    rows, bnd, dimg = rows[o], bnd[o], dimg[o]
    out_rows, out_bnd = [None] * bs, [None] * bs
    for b in range(bs):
        m = dimg == b
        if m.any():
            out_rows[b], out_bnd[b] = rows[m], bnd[m]
    return out_rows, out_bnd


def clustered(n, k, seed):
    """n boxes around k centres: the centres are oracle.riou.random_boxes(k, seed + 1000); every box takes a centre, N(0, 3 px) on cx and
    cy, a factor exp(N(0, 0.08)) on w and h, N(0, 0.05) on the angle, wrapped once by pi into (-pi/2, pi/2]; distinct scores
    (perm + 0.5) / n; sorted by score descending.  Near +-pi/2 the wrap puts members of one cluster on both ends of the angle range."""
    rng = np.random.default_rng(seed)
    centres = riou.random_boxes(k, seed + 1000)
    d = centres[rng.integers(0, k, n)].astype(np.float64)
    d[:, 0:2] += rng.normal(0, 3.0, (n, 2))
    d[:, 2:4] *= np.exp(rng.normal(0, 0.08, (n, 2)))
    d[:, 4] += rng.normal(0, 0.05, n)
    a = d[:, 4]
    a[a > np.pi / 2] -= np.pi
    a[a <= -np.pi / 2] += np.pi
    d[:, 5] = (rng.permutation(n) + 0.5) / n
    d = d.astype(np.float32)
    return d[np.argsort(-d[:, 5], kind='stable')]


def tile_pair_counts(d, thr, iou=None):
    """suppressing pairs (i < j, IoU > thr) per 64 x 64 tile of the upper triangle: what the mask kernel's summaries count"""
    d = np.ascontiguousarray(d, dtype=np.float32)
    n = len(d)
    if iou is None:
        iou = riou.riou_matrix(d, d)
    with np.errstate(invalid='ignore'):
        over = np.triu(iou > np.float32(thr), 1)
    W = (n + 63) // 64
    counts = {}
    for rb in range(W):
        for cb in range(rb, W):
            counts[(rb, cb)] = int(over[rb * 64:rb * 64 + 64, cb * 64:cb * 64 + 64].sum())
    return counts
