#!/usr/bin/env python
"""What the weighted merge costs on top of the plain segmented rotated NMS: r_nms_segmented against r_nms_merge_segmented (the same
call + the keep-word, owner and merge passes) on the same seeded inputs, in one process.

  (a) one segment of 50 000 boxes of oracle.riou.random_boxes' distribution (sparse: most tiles hold 0..7 suppressing pairs)
  (b) the same count around 2 000 cluster centres (tests/rnms_merge_reference.clustered: groups of ~25, dense tiles near the diagonal)
  (c) 16 images x 4 096 candidates, one segment per image

Per point: warm-up, then ROUNDS rounds; a round times K back-to-back plain calls and K merge calls, each batch between two device events,
K chosen so that a batch is at least 0.5 s of device work; the order inside a round alternates.  Printed: median and spread (min .. max)
of the per-call time of each, their difference, and the difference as a share of the plain call.

    python tools/nms_merge_bench.py [--rounds 5] [--min-seconds 0.5] > profiles/nms_merge.txt"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from oracle import riou  # noqa: E402
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.utils.nms.r_nms import r_nms_merge_segmented, r_nms_segmented  # noqa: E402
from tests.rnms_merge_reference import clustered  # noqa: E402


def _sorted(d):
    return d[np.argsort(-d[:, 5], kind="stable")]


def inputs():
    yield "(a) 1 x 50000 random_boxes", _sorted(riou.random_boxes(50000, seed=1)), [0, 50000]
    yield "(b) 1 x 50000 in 2000 clusters", clustered(50000, 2000, 7), [0, 50000]
    sets = [_sorted(riou.random_boxes(4096, seed=100 + k)) for k in range(16)]
    yield "(c) 16 x 4096 random_boxes", np.concatenate(sets), list(range(0, 16 * 4096 + 1, 4096))


def batch_ms(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--thr", type=float, default=0.3)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    print("# tools/nms_merge_bench.py: %s, library %s, thr %g, %d rounds, >= %g s of device work per timed batch"
          % (torch.cuda.get_device_name(0), _lib.lib().ryolo_build_id().decode(), opt.thr, opt.rounds, opt.min_seconds))
    print("# per-call milliseconds: median (min .. max) over the rounds; plain = r_nms_segmented, merge = r_nms_merge_segmented")
    for name, d, off in inputs():
        dets = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
        offs = torch.tensor(off, dtype=torch.int32, device=dev)
        max_len = int(np.diff(off).max())
        plain = lambda: r_nms_segmented(dets, offs, max_len, opt.thr)            # noqa: E731
        merge = lambda: r_nms_merge_segmented(dets, offs, max_len, opt.thr)      # noqa: E731
        flags = plain()
        f2, merged, owner = merge()
        assert torch.equal(flags, f2)
        kept = int(flags.sum())
        groups = int((torch.bincount(owner.long(), minlength=len(d)) > 1).sum())
        for fn in (plain, merge):
            batch_ms(fn, 3)
        k = max(1, int(np.ceil(opt.min_seconds * 1e3 / batch_ms(merge, 3))))
        tp, tm = [], []
        for r in range(opt.rounds):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (tm if which else tp).append(batch_ms(merge if which else plain, k))
        mp, mm = float(np.median(tp)), float(np.median(tm))
        print("%-32s kept %6d of %6d, %5d groups of more than one;  %d calls per batch" % (name, kept, len(d), groups, k))
        print("    plain %8.4f (%8.4f .. %8.4f)   merge %8.4f (%8.4f .. %8.4f)   difference %+8.4f ms = %+6.2f %% of the plain call"
              % (mp, min(tp), max(tp), mm, min(tm), max(tm), mm - mp, 100.0 * (mm - mp) / mp))


if __name__ == "__main__":
    main()
