"""GPU tier: the YOLO decode kernels (csrc/yolo.hip, csrc/yolo_decode.h) under every arc, on every kernel path, called through the C
ABI and compared with oracle.darknet_oracle.decode evaluated in float64.

One bar throughout: rtol = atol = 2e-5 against the float64 oracle -- the project's decode bar (tests/test_model_gpu.py,
test_decode_kernel_vs_oracle_and_golden), here against a reference that has no rounding of its own.  Non-finite values (exp overflow,
inf * 0, NaN logits) are compared as a pattern with the float32 oracle, which overflows where the kernels do.
"""
import math

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
import oracle
from oracle import darknet_oracle as do

pytestmark = pytest.mark.gpu
torch.set_num_threads(oracle.host_cores(16))

EINVAL = -1                       # RYOLO_EINVAL (include/ryolo.h)
ARC = {0: "default", 1: "uBCE", 2: "uCE"}
BS, NY, NX = 3, 5, 7              # 105 pixels: four 32-pixel tiles, the last one holds 9; tiles straddle the images at pixels 35 and 70
IMG = (NY * 16, NX * 16)          # stride = max(img) / max(nx, ny) = 16
STRIDE = 16.0
SENT = -12345.0
POISON = 777.0
BAR = dict(rtol=2e-5, atol=2e-5)
DEC_PIX, TILE_LIMIT = 32, 64 * 1024   # csrc/yolo.hip: pixels per tile, the tiled kernel's LDS limit


def _lib():
    from rotate_yolov3_amd import _lib as L
    return L


def _anchors(na):
    a = np.empty((na, 3), dtype=np.float32)
    a[:, 0] = 24 + 11 * np.arange(na)
    a[:, 1] = 9 + 5 * np.arange(na)
    a[:, 2] = np.linspace(-1.2, 1.2, na)
    return a


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _edge_head(na, no, seed):
    """[BS, na*no, NY, NX] bf16 head: randn * 1.5 plus the rows where a decode goes wrong.  Every logit is <= 80 or >= 92 in magnitude:
    nothing sits at the overflow edge of expf (88.7), so no assert depends on its last ulp."""
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(BS, na, no, NY, NX, generator=g) * 1.5).to(torch.bfloat16)
    h[0, 0, 2, 0, 0] = 20.0                       # first row of the first tile
    h[0, 1, 3, 1, 2] = -20.0
    h[1, 0, 2, 2, 3] = -20.0
    h[2, na - 1, 3, NY - 1, NX - 1] = 20.0        # last anchor of the last pixel (the 9-pixel tile)
    h[1, 1, 2, 3, 4] = 92.0                       # exp overflows in fp32: w = inf
    h[2, 0, 3, 0, 1] = 92.0                       # h = inf; w - inf * (cf - 1): NaN at cf 1 (inf * 0), -inf at cf 1.25
    h[2, 1, 2, 3, 3] = 92.0                       # w and h = inf: w = inf - inf = NaN under either cf
    h[2, 1, 3, 3, 3] = 92.0
    h[0, 2, no - 1, 2, 2] = float("nan")          # a NaN class logit (the last column)
    h[1, 2, 6, 4, 0] = float("nan")               # ... and the first class column
    return h.view(BS, na * no, NY, NX)


def _dev_head(head, dev, bs=BS):
    """the head as a channel slice (element offset 8) of a wider poisoned NHWC buffer: pixel stride = ceil8(C) + 8"""
    C = head.shape[1]
    cs = (C + 7) // 8 * 8 + 8
    wide = torch.full((bs, NY, NX, cs), POISON, dtype=torch.bfloat16)
    wide[..., 8:8 + C] = head.permute(0, 2, 3, 1)
    wide = wide.to(dev)
    return wide, wide[..., 8:8 + C], cs


def _tiled_expected(C, cs, ptr, no):
    """the host test of ryolo_yolo_decode that selects the tiled kernel (csrc/yolo.hip), restated"""
    return C % 8 == 0 and cs % 8 == 0 and ptr % 16 == 0 and DEC_PIX * C * 2 <= TILE_LIMIT and no <= 96


_ORACLE = {}


def _oracle(na, no, cf, arc):
    """float32 and float64 oracle of the edge head, computed once per (shape, cf, arc) and left unchanged"""
    key = (na, no, cf, arc)
    if key not in _ORACLE:
        head = _edge_head(na, no, 100 + na * no)
        a = _anchors(na)
        io32, p5 = do.decode(head.float(), a, IMG, cf=cf, arc=ARC[arc], nc=no - 6)
        io64, _ = do.decode(head.float(), a, IMG, cf=cf, arc=ARC[arc], nc=no - 6, dtype=torch.float64)
        _ORACLE[key] = (head, a, io32, io64, p5)
    return _ORACLE[key]


def _cmp_io(tag, got, io32, io64):
    """non-finite pattern == the float32 oracle's; every finite value inside the bar of the float64 oracle"""
    assert got.shape == io32.shape
    assert torch.equal(torch.isnan(got), torch.isnan(io32)), tag
    assert torch.equal(got == math.inf, io32 == math.inf) and torch.equal(got == -math.inf, io32 == -math.inf), tag
    f = torch.isfinite(io32)
    g, w = got[f].double(), io64[f]
    err = (g - w).abs()
    print("%s: %d finite values, %d non-finite; max abs err %.3g, max err / (atol + rtol |ref|) %.3g"
          % (tag, int(f.sum()), int((~f).sum()), float(err.max()), float((err / (BAR["atol"] + BAR["rtol"] * w.abs())).max())))
    assert np.allclose(g.numpy(), w.numpy(), **BAR), tag
    return int((~f).sum())


@pytest.mark.parametrize("cf", [1.0, 1.25])
@pytest.mark.parametrize("arc", [0, 1, 2])
@pytest.mark.parametrize("path,na,no", [("tiled<7>", 8, 7), ("tiled<0>", 8, 9), ("simple", 3, 7), ("simple", 3, 9)])
def test_decode_every_kernel_path_and_arc_vs_float64_oracle(cuda_dev, path, na, no, arc, cf):
    """ryolo_yolo_decode on the tiled kernel (single-class and generic instantiation) and on the simple kernel (C = 21 / 27: not a
    multiple of 8), arcs default / BCE / CE, context factor 1 and 1.25.  The path is not assumed: the host test that selects the tiled
    kernel is restated on the actual pointer and strides, and confirmed by the p-only form, which only the tiled kernel serves."""
    L = _lib()
    lib, dev = L.lib(), cuda_dev
    head, anchors, io32, io64, p5 = _oracle(na, no, cf, arc)
    C, n = na * no, na * NY * NX
    wide, hd, cs = _dev_head(head, dev)
    wide0 = wide.clone()
    tiled = _tiled_expected(C, cs, hd.data_ptr(), no)
    assert tiled == path.startswith("tiled") and (path != "tiled<7>" or no == 7) and (path != "tiled<0>" or no != 7)
    rows_img, row0 = 10 + n + 6, 10
    io = torch.full((BS, rows_img, no), SENT, device=dev)
    p = torch.full((BS, na, NY, NX, no), SENT, device=dev)
    a = torch.from_numpy(anchors).to(dev)
    rc = lib.ryolo_yolo_decode(hd.data_ptr(), cs, BS, NY, NX, na, no, a.data_ptr(), STRIDE, cf, arc, io.data_ptr(), rows_img, row0,
                               p.data_ptr(), L.stream_ptr(dev))
    assert rc == 0
    # the p-only form: served by the tiled kernel alone -- its return code says which kernel this shape takes
    p2 = torch.full((BS, na, NY, NX, no), SENT, device=dev)
    rc2 = lib.ryolo_yolo_decode(hd.data_ptr(), cs, BS, NY, NX, na, no, a.data_ptr(), STRIDE, cf, arc, None, rows_img, row0,
                                p2.data_ptr(), L.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc2 == (0 if tiled else EINVAL)
    assert _same_bits(p.cpu(), p5)                         # the head values, NaN payloads included
    if tiled:
        assert _same_bits(p2.cpu(), p5)
    else:
        assert bool((p2 == SENT).all())                    # refused before any launch
    io = io.cpu()
    nonfinite = _cmp_io("%s arc %d cf %g" % (path, arc, cf), io[:, row0:row0 + n], io32, io64)
    assert nonfinite >= 5                                  # the planted overflow / NaN rows are really there
    assert bool((io[:, :row0] == SENT).all()) and bool((io[:, row0 + n:] == SENT).all())
    assert torch.equal(wide.view(torch.int16), wide0.view(torch.int16))   # the head (and the poison around it) is only read
    if arc != 0:
        assert bool((io[:, row0:row0 + n, 5] == 1).all())
    if no == 7:
        assert bool((io[:, row0:row0 + n, 6] == 1).all())


def test_wide_heads_take_the_simple_kernel(cuda_dev):
    """a head whose 32-pixel tile exceeds 64 KiB (15 classes x 72 anchors = 1512 channels, 96 768 B) takes the simple kernel although
    its channel count is a multiple of 8: the p-only form is refused, the full form equals the float64 oracle (arc CE: the class loop
    of the simple kernel's own softmax over 15 columns)"""
    L = _lib()
    lib, dev = L.lib(), cuda_dev
    na, no, cf, arc, bs = 72, 21, 1.25, 2, 1
    g = torch.Generator().manual_seed(5)
    head = (torch.randn(bs, na * no, NY, NX, generator=g) * 1.5).to(torch.bfloat16)
    anchors = _anchors(na)
    io32, p5 = do.decode(head.float(), anchors, IMG, cf=cf, arc=ARC[arc], nc=no - 6)
    io64, _ = do.decode(head.float(), anchors, IMG, cf=cf, arc=ARC[arc], nc=no - 6, dtype=torch.float64)
    wide, hd, cs = _dev_head(head, dev, bs)
    C, n = na * no, na * NY * NX
    assert C % 8 == 0 and cs % 8 == 0 and hd.data_ptr() % 16 == 0 and DEC_PIX * C * 2 > TILE_LIMIT
    io = torch.full((bs, n + 3, no), SENT, device=dev)
    p = torch.full((bs, na, NY, NX, no), SENT, device=dev)
    a = torch.from_numpy(anchors).to(dev)
    assert lib.ryolo_yolo_decode(hd.data_ptr(), cs, bs, NY, NX, na, no, a.data_ptr(), STRIDE, cf, arc, None, n + 3, 3, p.data_ptr(),
                                 L.stream_ptr(dev)) == EINVAL
    assert lib.ryolo_yolo_decode(hd.data_ptr(), cs, bs, NY, NX, na, no, a.data_ptr(), STRIDE, cf, arc, io.data_ptr(), n + 3, 3,
                                 p.data_ptr(), L.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert _same_bits(p.cpu(), p5)
    io = io.cpu()
    _cmp_io("1512-channel head, simple kernel", io[:, 3:], io32, io64)
    assert bool((io[:, :3] == SENT).all())


# ---------------------------------------------------------------------------------------------------- decode + filter + compaction
F_BS, F_NA, MIN_WH, MARGIN = 2, 6, 2.0, 1e-4
F_ANCHORS = np.array([[30., 10., -0.6], [30., 10., 0.6], [60., 20., -0.6], [60., 20., 0.6], [90., 30., -0.6], [90., 30., 0.6]], dtype=np.float32)
F_THR = {0: 0.55, 1: 0.55, 2: 0.45}
# planted rows (image, anchor, y, x)
R_WOV, R_HOV, R_WHOV, R_CNAN = (0, 0, 0, 0), (0, 1, 0, 1), (0, 2, 0, 2), (0, 3, 0, 3)
R_OPINF, R_ONINF, R_ONAN = (0, 4, 1, 0), (0, 5, 1, 1), (1, 0, 1, 2)
R_WLO, R_WHI, R_HLO, R_HHI = (1, 1, 2, 0), (1, 2, 2, 1), (1, 3, 2, 2), (1, 4, 2, 3)
R_TIE0, R_TIE1 = (1, 5, 3, 0), (1, 0, 3, 1)


def _flat(r):
    b, a, y, x = r
    return b * (F_NA * NY * NX) + a * NY * NX + y * NX + x


_FILTER = {}


def _filter_case(arc, nc):
    """the seeded head of the filter test and what the reference keeps of it: oracle decode, then the filter half of
    non_max_suppression (utils/nms/nms.py:33-48).  CPU only; computed once per case."""
    if (arc, nc) in _FILTER:
        return _FILTER[(arc, nc)]
    no = nc + 6
    cf = 1.0 if nc == 1 else 1.25
    g = torch.Generator().manual_seed(40 + nc)
    h = torch.randn(F_BS, F_NA, no, NY, NX, generator=g) * 1.2
    h[:, :, 5] += 1.0                                            # some objectness above the threshold
    h = h.to(torch.bfloat16)

    def strong(r, cls=None, obj=3.0):
        """a row that survives on its score under every arc, with an ordinary box"""
        b, a, y, x = r
        h[b, a, 2:4, y, x] = 0.25
        h[b, a, 5, y, x] = obj
        h[b, a, 6:, y, x] = torch.tensor(cls if cls is not None else ([3.0] if nc == 1 else [-2.0, 4.0, -2.0])).to(torch.bfloat16)

    for r in (R_WOV, R_HOV, R_WHOV, R_CNAN, R_OPINF, R_ONINF, R_ONAN, R_WLO, R_WHI, R_HLO, R_HHI):
        strong(r)
    h[R_WOV[0], R_WOV[1], 2, R_WOV[2], R_WOV[3]] = 92.0
    h[R_HOV[0], R_HOV[1], 3, R_HOV[2], R_HOV[3]] = 92.0
    h[R_WHOV[0], R_WHOV[1], 2:4, R_WHOV[2], R_WHOV[3]] = 92.0
    h[R_CNAN[0], R_CNAN[1], no - 1, R_CNAN[2], R_CNAN[3]] = float("nan")
    h[R_OPINF[0], R_OPINF[1], 5, R_OPINF[2], R_OPINF[3]] = float("inf")
    h[R_ONINF[0], R_ONINF[1], 5, R_ONINF[2], R_ONINF[3]] = float("-inf")
    h[R_ONAN[0], R_ONAN[1], 5, R_ONAN[2], R_ONAN[3]] = float("nan")
    # w and h on either side of min_wh: h = exp(v3) * ah / cf;  w = exp(v2) * aw - h * (cf - 1) with the h of v3 = 0.25
    for r, t in ((R_WLO, 1.5), (R_WHI, 2.6)):
        aw, ah = float(F_ANCHORS[r[1], 0]), float(F_ANCHORS[r[1], 1])
        h[r[0], r[1], 2, r[2], r[3]] = math.log((t + math.exp(0.25) * ah / cf * (cf - 1)) / aw)
    for r, t in ((R_HLO, 1.5), (R_HHI, 2.6)):
        h[r[0], r[1], 3, r[2], r[3]] = math.log(t * cf / float(F_ANCHORS[r[1], 1]))
    if nc == 3:                                                  # tied class logits: the FIRST maximum is the class
        strong(R_TIE0, [6.0, 6.0, 0.0], obj=2.0)                 # (CE: each tied class holds 0.495 of the softmax, above its threshold)
        strong(R_TIE1, [0.0, 6.0, 6.0], obj=2.0)
    head = h.view(F_BS, F_NA * no, NY, NX)
    io32, _ = do.decode(head.float(), F_ANCHORS, IMG, cf=cf, arc=ARC[arc], nc=nc)
    io64, _ = do.decode(head.float(), F_ANCHORS, IMG, cf=cf, arc=ARC[arc], nc=nc, dtype=torch.float64)
    thr = F_THR[arc]

    def reduce(io):
        cls = io[..., 6:]
        cc = cls.max(2)[0]
        first = torch.where(cls == cc.unsqueeze(-1), torch.arange(nc).expand_as(cls), torch.full_like(cls, nc, dtype=torch.int64)).min(2)[0]
        return io[..., 5] * cc, cc, first

    score, cc, cls = reduce(io32)
    pred = io32.clone()
    pred[..., 5] = score                                         # nms.py: pred[:, 5] *= class_conf, then isfinite(pred).all(1)
    keep = (score > thr) & (io32[..., 2:4] > MIN_WH).all(2) & torch.isfinite(pred).all(2)

    def near(v, t):
        return torch.isfinite(v) & ((v - t).abs() <= MARGIN)
    maybe = near(score, thr) | near(io32[..., 2], MIN_WH) | near(io32[..., 3], MIN_WH)      # may fall either way
    s64, c64, _ = reduce(io64)
    want = torch.cat((io64[..., :5], s64.unsqueeze(-1), c64.unsqueeze(-1), cls.double().unsqueeze(-1)), 2).reshape(-1, 8)
    res = dict(head=head, no=no, cf=cf, thr=thr, io32=io32, keep=keep.flatten(), maybe=maybe.flatten(), want=want)
    res["sure"] = set(torch.nonzero(res["keep"] & ~res["maybe"]).flatten().tolist())
    res["allowed"] = set(torch.nonzero(res["keep"] | res["maybe"]).flatten().tolist())
    _FILTER[(arc, nc)] = res
    return res


def _check_filter_case(c, arc, nc):
    """the conditions the case must meet by the oracle alone"""
    total = c["keep"].numel()
    assert int(c["maybe"].sum()) <= 0.05 * total, "too many rows within the margin of a threshold"
    assert len(c["sure"]) > 20                                   # more than the capacity of the overflow run, too
    keep, w, hh = c["keep"], c["io32"][..., 2].flatten(), c["io32"][..., 3].flatten()
    for r in (R_WOV, R_HOV, R_WHOV, R_WLO, R_HLO):
        assert not keep[_flat(r)], r
    assert bool(keep[_flat(R_ONINF)]) == (arc != 0)              # sigmoid(-inf) = 0 under `default`; BCE / CE set the objectness to 1
    for r in (R_WHI, R_HHI):
        assert keep[_flat(r)], r
    assert 1.0 < w[_flat(R_WLO)] < MIN_WH - 0.1 and MIN_WH + 0.1 < w[_flat(R_WHI)] < 3.5
    assert 1.0 < hh[_flat(R_HLO)] < MIN_WH - 0.1 and MIN_WH + 0.1 < hh[_flat(R_HHI)] < 3.5
    # a NaN objectness: BCE overwrites it (io[..., 5] = 1) and the row survives; under `default` the score is NaN; under CE the softmax
    # over [objectness, classes] is NaN in every class column -- which the single-class overwrite io[..., 6] = 1 replaces again, so with
    # nc == 1 the row is finite and survives there as well (YOLOLayer.forward, model/models.py:237-246)
    assert bool(keep[_flat(R_ONAN)]) == (arc == 1 or (arc == 2 and nc == 1))
    # a NaN class logit fails the row unless the single-class overwrite replaces that column
    assert bool(keep[_flat(R_CNAN)]) == (nc == 1)
    if nc == 3:
        assert keep[_flat(R_TIE0)] and keep[_flat(R_TIE1)]
        assert c["want"][_flat(R_TIE0), 7] == 0 and c["want"][_flat(R_TIE1), 7] == 1


def _run_filter(L, dev, c, hd, cs, a, rows_img, row0, cand, rows, cnt, cap, arc):
    rc = L.lib().ryolo_yolo_decode_filter(hd.data_ptr(), cs, F_BS, NY, NX, F_NA, c["no"], a.data_ptr(), STRIDE, c["cf"], arc, c["thr"],
                                          MIN_WH, rows_img, row0, cand.data_ptr(), rows.data_ptr(), cnt.data_ptr(), cap,
                                          L.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    return int(cnt.item())


def _rows_of(tags, rows_img, row0, total):
    """cand_row tag = image * io_rows_per_image + io_row_offset + row  ->  index into the oracle's flattened [bs * total] rows"""
    out = []
    for t in tags:
        n, r = divmod(int(t), rows_img)
        r -= row0
        assert 0 <= n < F_BS and 0 <= r < total, t
        out.append(n * total + r)
    return out


def _check_values(c, ids, got):
    for r, row in zip(ids, got):
        want = c["want"][r]
        assert row[7] == want[7], (r, row, want)               # the class: first maximum
        assert np.allclose(row[:7].double().numpy(), want[:7].numpy(), **BAR), (r, row, want)


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("arc", [0, 1, 2])
def test_decode_filter_every_arc_nonfinite_rows_capacity_and_counter(cuda_dev, arc, nc):
    """ryolo_yolo_decode_filter against oracle decode + the filter half of non_max_suppression, on a head with overflowing w / h, NaN
    class logits, +inf / -inf / NaN objectness, boxes on either side of min_wh and tied class scores; then with a capacity the
    survivors exceed, and with a counter that starts above zero (the counter is shared by the heads of one forward).  Rows within 1e-4
    of a threshold (score, w, h) may fall either way, as in test_decode_filter_kernel_direct_vs_oracle; at most 5 % of rows are such."""
    L = _lib()
    dev = cuda_dev
    c = _filter_case(arc, nc)
    _check_filter_case(c, arc, nc)
    total = F_NA * NY * NX
    rows_img, row0 = total + 13, 7
    wide, hd, cs = _dev_head(c["head"], dev, F_BS)
    a = torch.from_numpy(F_ANCHORS).to(dev)
    sure, allowed = c["sure"], c["allowed"]

    # ---- room for everything
    cap = 1024
    cand = torch.full((cap, 8), SENT, device=dev)
    rows = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    m = _run_filter(L, dev, c, hd, cs, a, rows_img, row0, cand, rows, cnt, cap, arc)
    ids = _rows_of(rows[:m].cpu().tolist(), rows_img, row0, total)
    got = cand[:m].cpu()
    print("arc %d nc %d: %d survivors (oracle: %d sure, %d allowed, %d within the margin)" % (arc, nc, m, len(sure), len(allowed), int(c["maybe"].sum())))
    assert len(set(ids)) == m and sure <= set(ids) <= allowed
    assert bool((cand[m:] == SENT).all()) and bool((rows[m:] == -7).all())
    _check_values(c, ids, got)
    assert (_flat(R_ONAN) in ids) == (arc == 1 or (arc == 2 and nc == 1))
    if nc == 1 and arc != 0:
        # obj = 1 and the single class = 1: every finite row with w, h > min_wh scores exactly 1
        assert bool((got[:, 5] == 1).all()) and bool((got[:, 6] == 1).all()) and bool((got[:, 7] == 0).all())
        assert m >= int((torch.isfinite(c["io32"]).all(2) & (c["io32"][..., 2:4] > MIN_WH + MARGIN).all(2)).sum())

    # ---- capacity 16 < survivors: the counter still counts all, 16 distinct valid rows are written, nothing behind slot 15
    cand2 = torch.full((32, 8), SENT, device=dev)
    rows2 = torch.full((32,), -7, dtype=torch.int64, device=dev)
    cnt2 = torch.zeros(1, dtype=torch.int32, device=dev)
    m2 = _run_filter(L, dev, c, hd, cs, a, rows_img, row0, cand2, rows2, cnt2, 16, arc)
    assert m2 == m and m2 > 16
    ids2 = _rows_of(rows2[:16].cpu().tolist(), rows_img, row0, total)
    assert len(set(ids2)) == 16 and set(ids2) <= set(ids)
    _check_values(c, ids2, cand2[:16].cpu())
    assert bool((cand2[16:] == SENT).all()) and bool((rows2[16:] == -7).all())

    # ---- a counter that starts at 5: appended from slot 5, slots 0-4 are another head's
    cand3 = torch.full((cap, 8), SENT, device=dev)
    rows3 = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    cand3[:5] = 42.0
    rows3[:5] = -3
    cnt3 = torch.full((1,), 5, dtype=torch.int32, device=dev)
    m3 = _run_filter(L, dev, c, hd, cs, a, rows_img, row0, cand3, rows3, cnt3, cap, arc)
    assert m3 == 5 + m
    assert bool((cand3[:5] == 42.0).all()) and bool((rows3[:5] == -3).all())
    ids3 = _rows_of(rows3[5:m3].cpu().tolist(), rows_img, row0, total)
    assert sorted(ids3) == sorted(ids)
    _check_values(c, ids3, cand3[5:m3].cpu())
    assert bool((cand3[m3:] == SENT).all()) and bool((rows3[m3:] == -7).all())


# ---------------------------------------------------------------------------------------------------- the arc reaches every launch
@pytest.mark.parametrize("na_per_head", [72, 64])
@pytest.mark.parametrize("arc", ["uBCE", "uCE"])
def test_engine_passes_the_arc_to_every_decode_launch(cuda_dev, monkeypatch, arc, na_per_head):
    """Darknet-53 with 2 classes at 96^2, batch 2, built for a BCE / CE arc: the forward with the planner's default heads and with
    RYOLO_HEAD_DECODE=0 (conv, then ryolo_yolo_decode) are bit-identical; `io` is the float64 oracle decode of the returned p (the exact
    bf16 head), head by head with that head's anchors -- arc code, anchors, strides and row offsets; detect() (ryolo_yolo_decode_filter
    with the same arc) returns non_max_suppression(io).  72 anchors per head (the shipped cfg) x 8 columns is not a shape the fused
    head + decode launch serves (conv_pw_decode_supported: 1, 2 or 4 channel blocks), so that case runs conv + decode in both plans;
    with 64 anchors per head all three heads are fused launches (conv_pw.hip MODE 4) and the comparison is fused against unfused."""
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.utils.nms.nms import non_max_suppression
    from tests.procedural import fill_procedural
    hyp = {"context_factor": 1.0}
    cfg = make_cfg.darknet53(96, 96, classes=2, na_per_head=na_per_head)
    m = fill_procedural(Darknet(cfg, hyp, arc=arc).eval()).to(cuda_dev)
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(6)).to(cuda_dev)
    with torch.no_grad():
        io_a, p_a = m(x)
        io_a, p_a = io_a.clone(), [t.clone() for t in p_a]
        eng = [e for e in m._engines.values() if hasattr(e, "op_info")][0]
        assert eng.arc_code == (1 if arc == "uBCE" else 2)
        fused = sum(o["name"].endswith("+decode") for o in eng.op_info)
        assert fused == (3 if na_per_head == 64 else 0), [o["name"] for o in eng.op_info][-8:]
        score = io_a[..., 5] * io_a[..., 6:].max(2)[0]
        thr = float(score.flatten().kthvalue(int(score.numel() * 0.97)).values)
        det = eng.detect(x, thr, 0.3)
        want_det = non_max_suppression(io_a.clone(), thr, 0.3)
        monkeypatch.setenv("RYOLO_HEAD_DECODE", "0")
        m.refresh_engines()
        io_b, p_b = m(x)
        eng_b = [e for e in m._engines.values() if hasattr(e, "op_info")][0]
        assert not any(o["name"].endswith("+decode") for o in eng_b.op_info)
        assert sum(o["name"] == "yolo_decode" for o in eng_b.op_info) == 3
    torch.cuda.synchronize()
    assert torch.equal(io_a, io_b)
    for a, b in zip(p_a, p_b):
        assert torch.equal(a, b)
    # io == decode(p), per head
    yolos = [m.module_list[i] for i in m.yolo_layers]
    assert len(yolos) == 3 and all(y.na == na_per_head for y in yolos)
    ios = []
    for y, p in zip(yolos, p_a):
        bs, na, ny, nx, no = p.shape
        assert (na, no) == (na_per_head, 8)
        head = p.cpu().permute(0, 1, 4, 2, 3).reshape(bs, na * no, ny, nx)
        assert torch.equal(head, head.to(torch.bfloat16).float())           # p is the bf16 head
        ios.append(do.decode(head, y.anchors.cpu().numpy(), (96, 96), cf=1.0, arc=arc, nc=2, dtype=torch.float64)[0])
    io64 = torch.cat(ios, 1)
    got = io_a.cpu()
    assert got.shape == io64.shape and bool(torch.isfinite(got).all())
    err = (got.double() - io64).abs()
    print("%s na %d: io vs float64 decode of p: max abs err %.3g, max err / (atol + rtol |ref|) %.3g"
          % (arc, na_per_head, float(err.max()), float((err / (BAR["atol"] + BAR["rtol"] * io64.abs())).max())))
    assert np.allclose(got.double().numpy(), io64.numpy(), **BAR)
    assert bool((got[..., 5] == 1).all())
    # detect == NMS of io, row for row
    assert [d is None for d in det] == [w is None for w in want_det]
    for d, w in zip(det, want_det):
        if w is not None:
            assert torch.equal(d, w)
    assert sum(len(w) for w in want_det if w is not None) > 10
