"""r_nms -- mirror of the reference's native module `utils.nms.r_nms`
(utils/nms/src/rotate_polygon_nms.cpp:7-16; built by utils/nms/setup.py).

    r_nms(dets: Tensor[N,6] float32 on the GPU, threshold: float) -> LongTensor[K]

Same contract as the reference: columns (cx, cy, w, h, angle_rad, score); returns a new int64 tensor on dets'
device with the kept row indices in ascending order; N == 0 returns an empty int64 CPU tensor (cpp:9-10);
a non-GPU tensor raises RuntimeError like the reference's AT_CHECK (cpp:3,8).  `dets` may be a column slice
(utils/nms/nms.py:64 passes dc[:, :6] of an [n,8] tensor): the row stride is forwarded, nothing is copied.
The work happens in libryolo_hip.so (csrc/rnms.hip) through the C ABI `ryolo_rnms`; there is no CPU path.
"""
import torch

from ... import _lib


def _workspace(device, nbytes):
    """Scratch of ONE call, taken from torch's caching allocator on the current stream of `device` (the caller has made it the current
    device).  The allocator is stream-aware: the block returns to its pool when the tensor dies and is handed out again only to
    allocations on the same stream, behind this call in stream order -- so calls in flight on different streams or host threads never
    share scratch, and nothing a running call uses is ever dropped by a larger request elsewhere.  While the stream is being captured
    the block comes from the graph's private pool and lives as long as the graph.  A cache hit costs no host synchronisation."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def r_nms(dets, threshold):
    if not isinstance(dets, torch.Tensor) or not dets.is_cuda:
        raise RuntimeError("dets must be a CUDAtensor ")
    if dets.numel() == 0:
        return torch.empty(0, dtype=torch.long)
    if dets.dim() != 2 or dets.size(1) < 6:
        raise RuntimeError("dets must be [N, >=6] (cx, cy, w, h, angle, score)")
    if dets.dtype != torch.float32:
        dets = dets.float()
    if dets.stride(1) != 1 or dets.stride(0) < 6:
        dets = dets.contiguous()
    n = dets.size(0)
    L = _lib.lib()
    nbytes = L.ryolo_rnms_workspace_bytes(n)
    if nbytes == 0:
        _lib.check(-3, "ryolo_rnms")
    with torch.cuda.device(dets.device):
        ws = _workspace(dets.device, nbytes)
        keep = torch.empty(n, dtype=torch.long, device=dets.device)
        cnt = torch.empty(1, dtype=torch.int32, device=dets.device)
        rc = L.ryolo_rnms(dets.data_ptr(), n, dets.stride(0), float(threshold), keep.data_ptr(), cnt.data_ptr(),
                          ws.data_ptr(), ws.numel(), _lib.stream_ptr(dets.device))
        _lib.check(rc, "ryolo_rnms")
        k = int(cnt.item())   # the only host sync; the reference blocks on the whole n x n/64 mask instead
    return keep[:k]


def r_nms_segmented(dets, seg_offsets, max_seg_len, threshold):
    """Greedy rotated NMS of many independent sets in one launch (ryolo_rnms_segmented): rows [seg_offsets[s],
    seg_offsets[s+1]) of `dets` [M, >=6] are set s and must already be sorted by score, highest first.
    seg_offsets: int32 [S+1] on the device; max_seg_len: host int >= the longest set.  Returns uint8 keep flags [M]."""
    if not dets.is_cuda:
        raise RuntimeError("dets must be a CUDAtensor ")
    if dets.dtype != torch.float32 or dets.stride(1) != 1 or dets.stride(0) < 6:
        dets = dets.float().contiguous()
    m, S = dets.size(0), seg_offsets.numel() - 1
    flags = torch.zeros(m, dtype=torch.uint8, device=dets.device)
    if m == 0 or S <= 0:
        return flags
    seg_offsets = seg_offsets.to(device=dets.device, dtype=torch.int32).contiguous()
    L = _lib.lib()
    nbytes = L.ryolo_rnms_segmented_workspace_bytes(m, S, int(max_seg_len))
    if nbytes == 0:
        _lib.check(-3, "ryolo_rnms_segmented")
    with torch.cuda.device(dets.device):
        ws = _workspace(dets.device, nbytes)
        _lib.check(L.ryolo_rnms_segmented(dets.data_ptr(), m, dets.stride(0), seg_offsets.data_ptr(), S, int(max_seg_len),
                                          float(threshold), flags.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(dets.device)), "ryolo_rnms_segmented")
    return flags


def r_nms_merge_segmented(dets, seg_offsets, max_seg_len, threshold):
    """Weighted-merge rotated NMS of many independent sets in one call (ryolo_rnms_merge_segmented, include/ryolo.h): the input of
    r_nms_segmented.  Returns (flags uint8 [M]: exactly r_nms_segmented's; merged fp32 [M, 5]: for a kept row the score-weighted mean
    (cx, cy, w, h, a) of the rows it owns, itself included, zeros elsewhere; owner int32 [M]: the kept row a row belongs to, itself for a
    kept one)."""
    if not dets.is_cuda:
        raise RuntimeError("dets must be a CUDAtensor ")
    if dets.dtype != torch.float32 or dets.stride(1) != 1 or dets.stride(0) < 6:
        dets = dets.float().contiguous()
    m, S = dets.size(0), seg_offsets.numel() - 1
    flags = torch.zeros(m, dtype=torch.uint8, device=dets.device)
    merged = torch.zeros(m, 5, dtype=torch.float32, device=dets.device)
    owner = torch.arange(m, dtype=torch.int32, device=dets.device)
    if m == 0 or S <= 0:
        return flags, merged, owner
    seg_offsets = seg_offsets.to(device=dets.device, dtype=torch.int32).contiguous()
    L = _lib.lib()
    nbytes = L.ryolo_rnms_merge_segmented_workspace_bytes(m, S, int(max_seg_len))
    if nbytes == 0:
        _lib.check(-3, "ryolo_rnms_merge_segmented")
    with torch.cuda.device(dets.device):
        ws = _workspace(dets.device, nbytes)
        _lib.check(L.ryolo_rnms_merge_segmented(dets.data_ptr(), m, dets.stride(0), seg_offsets.data_ptr(), S, int(max_seg_len),
                                                float(threshold), flags.data_ptr(), owner.data_ptr(), merged.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _lib.stream_ptr(dets.device)),
                   "ryolo_rnms_merge_segmented")
    return flags, merged, owner


def riou_pairs(box1, box2):
    """IoU(box1[i], box2[i]) with the arithmetic of devRotateIoU (kernel.cu:251-260); rows (cx,cy,w,h,a,...)."""
    b1, b2 = _rows(box1), _rows(box2)
    assert b1.size(0) == b2.size(0)
    out = torch.empty(b1.size(0), dtype=torch.float32, device=b1.device)
    with torch.cuda.device(b1.device):
        rc = _lib.lib().ryolo_riou_pairs(b1.data_ptr(), b1.stride(0), b2.data_ptr(), b2.stride(0), b1.size(0),
                                         out.data_ptr(), _lib.stream_ptr(b1.device))
    _lib.check(rc, "ryolo_riou_pairs")
    return out


def riou_matrix(box1, box2):
    """out[i, j] = IoU(box1[i], box2[j])."""
    b1, b2 = _rows(box1), _rows(box2)
    out = torch.empty(b1.size(0), b2.size(0), dtype=torch.float32, device=b1.device)
    with torch.cuda.device(b1.device):
        rc = _lib.lib().ryolo_riou_matrix(b1.data_ptr(), b1.size(0), b1.stride(0), b2.data_ptr(), b2.size(0),
                                          b2.stride(0), out.data_ptr(), _lib.stream_ptr(b1.device))
    _lib.check(rc, "ryolo_riou_matrix")
    return out


def skew_iou_pairs(box1, box2):
    """IoU(box1[i], box2[i]) of the evaluation path (reference utils.py:290-320: exact polygon IoU in fp64)."""
    b1, b2 = _rows(box1), _rows(box2)
    assert b1.size(0) == b2.size(0)
    out = torch.empty(b1.size(0), dtype=torch.float32, device=b1.device)
    with torch.cuda.device(b1.device):
        rc = _lib.lib().ryolo_skew_iou_pairs(b1.data_ptr(), b1.stride(0), b2.data_ptr(), b2.stride(0), b1.size(0),
                                             out.data_ptr(), _lib.stream_ptr(b1.device))
    _lib.check(rc, "ryolo_skew_iou_pairs")
    return out


def skew_iou_matrix(box1, box2):
    """out[i, j] = evaluation-path IoU(box1[i], box2[j])."""
    b1, b2 = _rows(box1), _rows(box2)
    out = torch.empty(b1.size(0), b2.size(0), dtype=torch.float32, device=b1.device)
    with torch.cuda.device(b1.device):
        rc = _lib.lib().ryolo_skew_iou_matrix(b1.data_ptr(), b1.size(0), b1.stride(0), b2.data_ptr(), b2.size(0),
                                              b2.stride(0), out.data_ptr(), _lib.stream_ptr(b1.device))
    _lib.check(rc, "ryolo_skew_iou_matrix")
    return out


def eval_match(det, det_off, lab, lab_off, iou_thres):
    """mAP matching of a whole batch in one call (ryolo_eval_match: three launches, no host read).  det [M, >=8] rows (x, y, w, h, a,
    score, cls_conf, cls) of all images, image after image and score-descending inside an image; det_off int32 [n_img+1] on the device;
    lab [T, >=6] rows (cls, x, y, w, h, a) in pixels in image order, lab_off likewise.  Returns (correct uint8 [M], matched int32 [M]: the
    row of `lab` a correct prediction detected, else -1) on the device -- per image exactly what the greedy loop of
    metrics.match_predictions marks."""
    det, lab = _rows(det, 8, "det"), _rows(lab, 6, "lab")
    m, t, n_img = det.size(0), lab.size(0), det_off.numel() - 1
    if lab_off.numel() != n_img + 1 or n_img < 0:
        raise RuntimeError("det_off and lab_off must both hold n_img + 1 offsets")
    correct = torch.empty(m, dtype=torch.uint8, device=det.device)
    matched = torch.empty(m, dtype=torch.int32, device=det.device)
    if m == 0:
        return correct, matched
    det_off = det_off.to(device=det.device, dtype=torch.int32).contiguous()
    lab_off = lab_off.to(device=det.device, dtype=torch.int32).contiguous()
    L = _lib.lib()
    with torch.cuda.device(det.device):
        ws = _workspace(det.device, L.ryolo_eval_match_workspace_bytes(m, t))
        rc = L.ryolo_eval_match(det.data_ptr(), det.stride(0), det_off.data_ptr(), lab.data_ptr(), lab.stride(0), lab_off.data_ptr(),
                                n_img, m, t, float(iou_thres), correct.data_ptr(), matched.data_ptr(), ws.data_ptr(), ws.numel(),
                                _lib.stream_ptr(det.device))
    _lib.check(rc, "ryolo_eval_match")
    return correct, matched


def _rows(b, cols=5, what="boxes"):
    if not b.is_cuda:
        raise RuntimeError("%s must be a CUDAtensor " % what)
    if b.dim() != 2 or b.size(1) < cols:
        raise RuntimeError("%s must be [N, >=%d]" % (what, cols))
    if b.dtype != torch.float32:
        b = b.float()
    if b.stride(1) != 1 or b.stride(0) < cols:
        b = b.contiguous()
    return b
