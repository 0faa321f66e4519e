"""Oracle of ryolo_letterbox_area: the definition in the header comment of csrc/letterbox_area.hip, restated with numpy.

letterbox_area(images, src, place, H, W, dtype) evaluates it in `dtype`: float64 is the oracle; float32 performs the kernel's own
operations in the kernel's own order (numpy's float32 +, *, / are IEEE, the unit is built without contraction), and the difference of
the two on a test's inputs measures the rounding the comparison has to allow.  The integer tap lists are exact in both."""
import numpy as np


def taps(k, s, n):
    """-> (indices, integer weights, divisor) of output index k on an axis of source length s and output length n"""
    k, s, n = int(k), int(s), int(n)
    if n < s:
        idx, wts = [], []
        i = (k * s) // n
        while i * n < (k + 1) * s:
            idx.append(i)
            wts.append(min((k + 1) * s, (i + 1) * n) - max(k * s, i * n))
            i += 1
        assert sum(wts) == s and all(w > 0 for w in wts) and idx[-1] <= s - 1
        return idx, wts, s
    c = (2 * k + 1) * s - n
    q, r = c // (2 * n), c % (2 * n)                  # Python's floor division and its non-negative remainder
    return [min(max(q, 0), s - 1), min(max(q + 1, 0), s - 1)], [2 * n - r, r], 2 * n


def letterbox_area(images, src, place, H, W, dtype=np.float64):
    """-> [N, H, W, 3] in [0, 1] units (before the bf16 rounding), in `dtype`"""
    f = dtype
    out = np.empty((len(src), H, W, 3), dtype=f)
    out[:] = f(128) / f(255)
    for n, (s, (left, top, new_w, new_h)) in enumerate(zip(src, place)):
        if not 0 <= s < len(images):
            continue
        img = images[s].astype(f)
        h, w = img.shape[:2]
        xt = [taps(k, w, new_w) for k in range(new_w)]
        yt = [taps(k, h, new_h) for k in range(new_h)]
        # rows[iy][k]: the horizontal sums of source row iy, only for the source rows some output row uses
        need = sorted(set(i for idx, _, _ in yt for i in idx))
        rows = {}
        for iy in need:
            r = np.empty((new_w, 3), dtype=f)
            for k, (idx, wts, D) in enumerate(xt):
                acc = f(wts[0]) * img[iy, idx[0]]
                for i, wt in zip(idx[1:], wts[1:]):
                    acc = acc + f(wt) * img[iy, i]
                r[k] = acc / f(D)
            rows[iy] = r
        for ky, (idx, wts, D) in enumerate(yt):
            acc = f(wts[0]) * rows[idx[0]]
            for i, wt in zip(idx[1:], wts[1:]):
                acc = acc + f(wt) * rows[i]
            out[n, top + ky, left:left + new_w] = (acc / f(D)) / f(255)
    return out
