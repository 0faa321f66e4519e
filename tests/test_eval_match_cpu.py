"""CPU tier: the batched mAP matcher (ryolo_eval_match, include/ryolo.h) as far as it goes without a GPU -- the two symbols are declared
and exported, every RYOLO_EINVAL case returns before anything is enqueued, and the first-claimant rule the kernels implement (DESIGN.md
section 3.7; tests/eval_match_ref.py states it in numpy and checks the GPU results with it) equals the literal greedy loop."""
import ctypes as C
import os
import re

import numpy as np

from tests.eval_match_ref import first_claimant, literal_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _lib():
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    import rotate_yolov3_amd  # noqa: F401
    from rotate_yolov3_amd import _lib as binding
    return binding.lib()


def test_header_declares_and_library_exports_the_matcher():
    src = open(os.path.join(ROOT, "include", "ryolo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib()
    for name in ("ryolo_eval_match_workspace_bytes", "ryolo_eval_match"):
        assert re.search(r"\b%s\s*\(" % name, src), "include/ryolo.h does not declare %s" % name
        assert hasattr(lib, name), "libryolo_hip.so does not export %s" % name
    import rotate_yolov3_amd  # noqa: F401
    from rotate_yolov3_amd import _lib as binding
    assert "ryolo_eval_match" in binding._sigs and "ryolo_eval_match_workspace_bytes" in binding._sigs


def test_argument_validation_without_gpu():
    lib = _lib()
    vp = C.c_void_p
    ws_bytes, f = lib.ryolo_eval_match_workspace_bytes, lib.ryolo_eval_match
    p = vp(4096)                        # never dereferenced: every call below returns from the host-side checks
    big = 1 << 20

    def call(det=p, det_stride=8, det_off=p, lab=p, lab_stride=6, lab_off=p, n_img=1, n_det=4, n_lab=2, thres=0.5, correct=p,
             matched=None, ws=p, nbytes=big):
        return f(det, det_stride, det_off, lab, lab_stride, lab_off, n_img, n_det, n_lab, thres, correct, matched, ws, nbytes, None)

    assert call(n_det=-1) == EINVAL and call(n_lab=-1) == EINVAL and call(n_img=-1) == EINVAL
    assert call(det_stride=7) == EINVAL and call(lab_stride=5) == EINVAL
    assert call(thres=float("nan")) == EINVAL and call(thres=-0.25) == EINVAL and call(thres=1.0) == EINVAL
    assert call(nbytes=ws_bytes(4, 2) - 1) == EINVAL
    assert call(correct=None) == EINVAL and call(det=None) == EINVAL and call(det_off=None) == EINVAL
    assert call(lab=None) == EINVAL and call(lab_off=None) == EINVAL and call(ws=None) == EINVAL and call(ws=vp(4100)) == EINVAL
    assert call(n_img=0) == EINVAL                                      # predictions that belong to no image
    # nothing to do is not an error, and needs no pointer at all
    assert f(None, 8, None, None, 6, None, 0, 0, 0, 0.5, None, None, None, 0, None) == 0
    assert f(None, 8, None, p, 6, p, 3, 0, 5, 0.0, None, None, None, ws_bytes(0, 5), None) == 0
    # the workspace query: finite, and monotone in both arguments
    assert ws_bytes(0, 0) < big and ws_bytes(-1, 3) == 0 and ws_bytes(3, -1) == 0
    sizes = [0, 1, 2, 63, 64, 65, 1000, 70000, 1 << 24]
    for a, b in zip(sizes[:-1], sizes[1:]):
        for other in (0, 7, 5000):
            assert ws_bytes(a, other) < ws_bytes(b, other) and ws_bytes(other, a) < ws_bytes(other, b)
    assert ws_bytes(2 ** 31 - 1, 2 ** 31 - 1) > 2 ** 37                  # no 32-bit overflow


def test_first_claimant_rule_equals_the_literal_loop():
    """12 000 random cases, 0-12 predictions x 0-6 labels x 3 classes; IoU values from a small set so that ties at the maximum and values
    AT the threshold are common -- among them fp32(0.1), which is > 0.1 as a double and not as a float: the loop compares in fp32."""
    rng = np.random.RandomState(2024)
    values = np.array([0.0, 0.1, 0.25, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.75, 1.0], dtype=np.float32)
    ties = at_thres = corrects = taken = 0
    for case in range(12000):
        n, nl = rng.randint(0, 13), rng.randint(0, 7)
        iou = values[rng.randint(0, len(values), (n, nl))]
        pcls, tcls = rng.randint(0, 3, n).astype(np.float32), rng.randint(0, 3, nl).astype(np.float32)
        thres = [0.5, 0.25, 0.1, 0.0][case % 4]
        want_c, want_m = literal_loop(iou, pcls, tcls, thres)
        got_c, got_m = first_claimant(iou, pcls, tcls, thres)
        assert got_c.tolist() == want_c and got_m.tolist() == want_m, (case, iou, pcls, tcls, thres)
        if n and nl:
            v = np.where(pcls[:, None] == tcls[None, :], iou, -1)
            mx = v.max(1)
            ties += int(((v == mx[:, None]).sum(1) >= 2)[mx > 0].sum())
            at_thres += int((mx == np.float32(thres)).sum())
            claims = mx > np.float32(thres)
            corrects += int(got_c.sum())
            taken += int(claims.sum() - got_c.sum())
    assert ties > 2000 and at_thres > 3000 and corrects > 10000 and taken > 5000, (ties, at_thres, corrects, taken)


def test_flat_rows_of_the_nms_wrapper_without_detections():
    """non_max_suppression_batched(flat=True) hands out (list, flat rows, int32 offsets) also where it returns early, and the default
    return value is the list alone"""
    import torch
    import rotate_yolov3_amd  # noqa: F401
    from rotate_yolov3_amd.utils.nms import nms
    empty = torch.zeros(3, 0, 8)
    assert nms.non_max_suppression_batched(empty.clone(), 0.5, 0.5) == [None] * 3
    output, det, det_off = nms.non_max_suppression_batched(empty.clone(), 0.5, 0.5, flat=True)
    assert output == [None] * 3 and det.shape == (0, 8) and det_off.tolist() == [0] * 4 and det_off.dtype == torch.int32
    rows = [None, torch.arange(24.0).view(3, 8), None, torch.ones(2, 8)]
    det, det_off = nms._flat(rows, torch.device("cpu"))
    assert det_off.tolist() == [0, 0, 3, 3, 5] and torch.equal(det[:3], rows[1]) and torch.equal(det[3:], rows[3])
