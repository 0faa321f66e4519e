"""Shared by tests/test_eval_match_cpu.py and tests/test_eval_match_gpu.py: the greedy matching loop of the reference's test.py:121-151
transcribed literally, the first-claimant rule as a numpy checker, and the seeded batch the GPU tests run."""
import numpy as np
import torch

# (predictions, labels) per image of the GPU batch: an empty leading image, labels without predictions, predictions without labels, one
# pair, a wave of 63, 65 (two waves), 257 (past 256 lanes), and 300 predictions on 3 labels
BATCH_COUNTS = [(0, 0), (0, 4), (5, 0), (1, 1), (63, 7), (65, 40), (257, 130), (300, 3)]
# chosen on the CPU (oracle/poly_iou.py IoUs, the literal loop) so that every kind of prediction the GPU test asks for occurs:
# python tests/eval_match_ref.py
BATCH_SEED = 0


def literal_loop(iou, pcls, tcls, thres):
    """test.py:121-151 (as utils/metrics.py:match_predictions restates it) on CPU tensors: iou fp32 [n, nl], pcls [n], tcls [nl].
    Returns (correct [n] 0/1, matched [n]: the detected label or -1)."""
    iou, pcls, tcls = torch.as_tensor(iou, dtype=torch.float32), torch.as_tensor(pcls), torch.as_tensor(tcls)
    n, nl = len(pcls), len(tcls)
    correct, matched = [0] * n, [-1] * n
    if nl == 0 or n == 0:
        return correct, matched
    detected = []
    for i in range(n):
        if len(detected) == nl:
            break
        m = (pcls[i] == tcls).nonzero().view(-1)
        if len(m) == 0:
            continue
        v, bi = iou[i, m].max(0)
        if v > thres and int(m[bi]) not in detected:
            correct[i] = 1
            matched[i] = int(m[bi])
            detected.append(int(m[bi]))
    return correct, matched


def first_claimant(iou, pcls, tcls, thres, pimg=None, timg=None):
    """The rule: prediction i is correct iff its best same-class label (largest fp32 IoU, lowest index on ties) has IoU > fp32(thres) and
    no smaller i claims the same label.  With pimg / timg (image of every prediction / label) a label is a candidate only for the
    predictions of its own image, so one call checks a whole batch.  Returns (correct uint8 [n], matched int64 [n])."""
    iou = np.asarray(iou, dtype=np.float32)
    pcls, tcls = np.asarray(pcls), np.asarray(tcls)
    n, nl = len(pcls), len(tcls)
    correct, matched = np.zeros(n, np.uint8), np.full(n, -1, np.int64)
    if n == 0 or nl == 0:
        return correct, matched
    same = pcls[:, None] == tcls[None, :]
    if pimg is not None:
        same &= np.asarray(pimg)[:, None] == np.asarray(timg)[None, :]
    v = np.where(same, iou.reshape(n, nl), -np.inf).astype(np.float32)
    best = v.argmax(1)                                   # the first maximum: lowest label index
    rows = np.arange(n)
    claim = same.any(1) & (v[rows, best] > np.float32(thres))
    first = np.full(nl, n, np.int64)
    np.minimum.at(first, best[claim], rows[claim])
    ok = claim & (first[best] == rows)
    correct[ok] = 1
    matched[ok] = best[ok]
    return correct, matched


def make_batch(seed, counts=BATCH_COUNTS, classes=3):
    """Predictions as tests/golden/gen_eval_golden.py builds them: jittered copies of labels (jitter scales 0.15 / 0.4 / 1.2, 20 % with a
    wrong class) plus random background, score-descending per image; labels 1 and 0 of image 5 are exact duplicates.
    Returns (det [M,8], det_off [n_img+1], lab [T,6], lab_off [n_img+1]) as numpy arrays."""
    r = np.random.RandomState(seed)
    dets, labs = [], []
    for im, (k, nl) in enumerate(counts):
        lab = np.zeros((nl, 6), dtype=np.float32)
        if nl:
            lab[:, 0] = r.randint(0, classes, nl)
            lab[:, 1:3] = r.uniform(80, 520, (nl, 2))
            lab[:, 3] = r.uniform(60, 160, nl)
            lab[:, 4] = lab[:, 3] / r.uniform(3, 8, nl)
            lab[:, 5] = r.uniform(-1.5, 1.5, nl)
        if im == 5 and nl > 1:
            lab[1] = lab[0]
        pred = np.zeros((k, 8), dtype=np.float32)
        for i in range(k):
            if nl and i < 0.8 * k:
                t = lab[r.randint(0, nl)]
                pred[i, :5] = t[1:6] + r.normal(0, 1, 5) * np.array([6, 6, 8, 3, 0.08]) * r.choice([0.15, 0.4, 1.2])
                pred[i, 7] = t[0] if r.rand() < 0.8 else (t[0] + 1) % classes
            else:
                pred[i, :5] = [r.uniform(50, 550), r.uniform(50, 550), r.uniform(40, 120), r.uniform(8, 30), r.uniform(-1.5, 1.5)]
                pred[i, 7] = r.randint(0, classes)
            pred[i, 5] = r.uniform(0.05, 0.99)
            pred[i, 6] = 1.0
        dets.append(pred[np.argsort(-pred[:, 5], kind="stable")])
        labs.append(lab)
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum([len(x) for x in labs])]).astype(np.int32)
    return np.concatenate(dets).astype(np.float32), det_off, np.concatenate(labs).astype(np.float32), lab_off


def kinds(iou, pcls, tcls, correct, thres):
    """Per prediction of ONE image: 0 correct, 1 best label above the threshold but already claimed, 2 same-class label present but best
    IoU <= threshold, 3 no same-class label; and whether its maximum over the same-class labels is positive and attained twice."""
    iou = np.asarray(iou, dtype=np.float32)
    n = len(pcls)
    kind, tie = np.full(n, 3), np.zeros(n, bool)
    if len(tcls) == 0:
        return kind, tie
    same = np.asarray(pcls)[:, None] == np.asarray(tcls)[None, :]
    v = np.where(same, iou, -np.inf).astype(np.float32)
    mx = v.max(1)
    has = same.any(1)
    kind[has & (mx <= np.float32(thres))] = 2
    kind[has & (mx > np.float32(thres))] = 1
    kind[np.asarray(correct, bool)] = 0
    tie = has & (mx > 0) & ((v == mx[:, None]).sum(1) >= 2)
    return kind, tie


def batch_is_not_trivial(det, det_off, lab, lab_off, iou_of, thres):
    """Asserts what the GPU test asks of its inputs; iou_of(boxes1 [n,5], boxes2 [m,5]) -> fp32 [n, m].  Returns the share of correct."""
    seen, ties, n_correct = set(), 0, 0
    for im in range(len(det_off) - 1):
        p, t = det[det_off[im]:det_off[im + 1]], lab[lab_off[im]:lab_off[im + 1]]
        if len(p) == 0:
            continue
        iou = iou_of(p[:, :5], t[:, 1:6]) if len(t) else np.zeros((len(p), 0), np.float32)
        correct, _ = literal_loop(iou, p[:, 7], t[:, 0], thres)
        kind, tie = kinds(iou, p[:, 7], t[:, 0], correct, thres)
        seen |= set(kind.tolist())
        ties += int(tie.sum())
        n_correct += int(np.sum(correct))
    assert seen == {0, 1, 2, 3}, seen
    assert ties >= 1
    share = n_correct / float(len(det))
    assert 0.1 <= share <= 0.9, share
    return share


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import poly_iou

    def cpu_iou(b1, b2):
        out = np.zeros((len(b1), len(b2)), np.float32)
        r1, r2 = 0.5 * np.hypot(b1[:, 2], b1[:, 3]), 0.5 * np.hypot(b2[:, 2], b2[:, 3])
        c2 = [poly_iou.get_rotated_coors(b.astype(np.float64)) for b in b2]
        for i, a in enumerate(b1):
            ca = poly_iou.get_rotated_coors(a.astype(np.float64))
            for j in np.flatnonzero(np.hypot(b2[:, 0] - a[0], b2[:, 1] - a[1]) <= (r1[i] + r2) * 1.001 + 1e-3):   # others: disjoint, 0
                out[i, j] = poly_iou.skewiou(ca, c2[j])
        return out

    for seed in range(100):
        try:
            print("seed", seed, "share correct %.3f" % batch_is_not_trivial(*make_batch(seed), iou_of=cpu_iou, thres=0.5))
            break
        except AssertionError as e:
            print("seed", seed, "rejected:", e)
