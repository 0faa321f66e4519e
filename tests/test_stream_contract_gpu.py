"""GPU tier: the STREAM contract of the C ABI's detection half (include/ryolo.h: "every function only ENQUEUES work on `stream`",
"hipGraph-capturable", and for ryolo_rnms on more than 20 416 boxes "everything after it sees its results" although part of the call
runs on a library-owned second stream).  The arithmetic is held by test_rnms_gpu.py / test_skewiou_gpu.py / test_model_gpu.py on
torch's default stream, eagerly, from one host thread; here the same bit-exact references are asked on side streams without a host
synchronisation in between, from captured graphs replayed on new contents, and from two host threads at once.

Every NMS call of sections a - c goes through the C ABI with caller-owned keep / count / workspace tensors and an explicit stream
pointer (the Python r_nms ends in .item() and cannot be captured); section d tests the Python wrappers.  References: oracle.riou.rnms
(bit-exact) and, at 50 000 boxes, the committed SHA of tests/golden/rnms_keep_n50000.npz.

What each test would have caught in the code before it (csrc/rnms.hip / utils/nms/r_nms.py as of ABI version 2):
  b  side_pool() asked hipStreamIsCapturing only while the pool did not exist (rnms.hip:945): once an eager large call had created it,
     a large call on a capturing stream forked onto the process-wide second stream -- that stream joined the capture, the graph got
     two parallel branches, and an eager large call made meanwhile was captured into the wrong graph or broke the capture.
  c  the same shared stream + two events under two host threads (rnms.hip:1022-1039).
  d  one scratch tensor per device whatever the stream (r_nms.py:20-24): two calls in flight wrote the same tiles / summaries, and a
     larger request dropped the tensor a call on another stream was still using.
"""
import functools
import hashlib
import os
import threading

import numpy as np
import pytest
import torch

import oracle
from oracle import poly_iou as pi
from oracle import riou
from tests.box_pairs import clustered_boxes

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = 0.45
WAVE, PANEL = 64, 4                      # csrc/rnms.hip: boxes per block row, block rows per scan panel
# (n, seed of the cluster draws, seed of the background boxes); A and B are the two contents of the capture / thread tests
CASE_A = (26000, 9001, 101)
CASE_B = (26000, 9002, 102)


@pytest.fixture(scope="module")
def L(cuda_dev):
    import rotate_yolov3_amd  # noqa: F401
    from rotate_yolov3_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _case(n, seed, bg_seed):
    """clustered boxes + the oracle's keep list (one oracle run per case for the whole file)"""
    d = clustered_boxes(n, np.random.default_rng(seed), bg_seed=bg_seed)
    return d, riou.rnms(d, THR, nthreads=oracle.host_cores(8))


def split_handoff_matters(d, want, thr=THR):
    """CPU only.  With the boxes in the order the scan visits them and k = the first box of the second mask launch of a split call
    (csrc/rnms.hip: k = (ceil(W / 4) * 3 // 5) * 4 block rows): does NMS of the two parts on their own differ from NMS of the whole,
    i.e. do boxes kept in the first part suppress boxes of the second?  Only then does a lost or early hand-off between the pieces of
    a split call change the keep list."""
    n = len(d)
    W = (n + WAVE - 1) // WAVE
    k = ((W + PANEL - 1) // PANEL * 3 // 5) * PANEL * WAVE
    assert 0 < k < n
    o = np.argsort(-d[:, 5], kind="stable")
    ds = d[o]
    inv = np.empty(n, np.int64)
    inv[o] = np.arange(n)
    whole = np.sort(inv[want])                                           # the oracle's keep list as positions in the sorted order
    nt = oracle.host_cores(8)
    parts = np.concatenate([np.sort(riou.rnms(ds[:k], thr, nthreads=nt)), k + np.sort(riou.rnms(ds[k:], thr, nthreads=nt))])
    assert np.array_equal(parts[parts < k], whole[whole < k])            # the first part never depends on the second
    return len(parts) > len(whole) and not np.array_equal(parts, whole)


def _pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


class NmsCall(object):
    """caller-owned buffers of one ryolo_rnms call of n boxes"""

    def __init__(self, L, n, dev):
        self.L, self.n = L, n
        self.dets = torch.zeros(n, 6, device=dev)
        self.keep = torch.empty(n, dtype=torch.int64, device=dev)
        self.cnt = torch.empty(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(L.lib().ryolo_rnms_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def poison(self):
        """on the current stream: results of an earlier call cannot pass for this one's"""
        self.keep.fill_(-1)
        self.cnt.fill_(-1)

    def enqueue(self, stream):
        return self.L.lib().ryolo_rnms(self.dets.data_ptr(), self.n, 6, THR, self.keep.data_ptr(), self.cnt.data_ptr(),
                                       self.ws.data_ptr(), self.ws.numel(), stream.cuda_stream)

    def result(self):
        k = int(self.cnt.item())
        assert 0 <= k <= self.n, k
        return self.keep[:k].cpu().numpy()


# ------------------------------------------------------------------------------------------------ a. a side stream, no host sync
@pytest.mark.parametrize("n,seed,bg_seed", [(20416, 9003, 103), (20417, 9004, 104), CASE_A])
def test_rnms_on_a_side_stream_without_host_sync(L, cuda_dev, n, seed, bg_seed):
    """Upload, ryolo_rnms and a dependent op back to back on a stream of the test's own, one synchronisation at the end: the last
    unsplit size, the first split one and 26 000 boxes.  The split call's second stream has no implicit ordering with this stream (it
    is non-blocking, and this is not the null stream): only the call's own events make the upload visible to it and its rows to what
    follows."""
    d, want = _case(n, seed, bg_seed)
    host = _pinned(d)
    call = NmsCall(L, n, cuda_dev)
    s = torch.cuda.Stream(cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    with torch.cuda.stream(s):
        call.poison()
        call.dets.copy_(host, non_blocking=True)
        rc = call.enqueue(s)
        head = call.keep[:8].clone()
        k = call.cnt.clone()
    assert rc == 0, L.lib().ryolo_strerror(rc)
    s.synchronize()
    assert int(k.item()) == len(want)
    assert np.array_equal(head.cpu().numpy(), want[:8])
    assert np.array_equal(call.result(), want)


# ------------------------------------------------------------------------------------------------ b. capture and replay
def test_rnms_captured_after_the_side_pool_exists_replays_on_new_contents(L, cuda_dev):
    """First one EAGER 26 000-box call (it creates the library's second stream and events), then a 26 000-box ryolo_rnms captured on a
    side stream: the captured call must run unsplit, as a linear chain on the capturing stream.  Ten replays: contents A, B, A (new
    contents at the same pointers give the new answer: extent, sort and scan state are recomputed on the device, nothing was baked
    in at capture), then seven more on A equal to the first; between two of them an eager split call on the default stream, which
    uses the shared second stream and must neither disturb nor be disturbed by the graph."""
    (da, wa), (db, wb) = _case(*CASE_A), _case(*CASE_B)
    assert not np.array_equal(wa, wb)
    assert split_handoff_matters(da, wa) and split_handoff_matters(db, wb)
    eager = NmsCall(L, len(da), cuda_dev)
    eager.dets.copy_(torch.from_numpy(da))
    eager.poison()
    assert eager.enqueue(torch.cuda.current_stream(cuda_dev)) == 0
    torch.cuda.synchronize(cuda_dev)
    assert np.array_equal(eager.result(), wa)

    cap = NmsCall(L, len(da), cuda_dev)
    cap.dets.copy_(torch.from_numpy(da))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        rc = cap.enqueue(torch.cuda.current_stream(cuda_dev))
    assert rc == 0, L.lib().ryolo_strerror(rc)

    def replay(d):
        cap.dets.copy_(torch.from_numpy(d))
        cap.poison()
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        return cap.result()

    first = replay(da)
    assert np.array_equal(first, wa)
    assert np.array_equal(replay(db), wb)
    assert np.array_equal(replay(da), wa)
    for i in range(7):
        if i == 3:
            eager.dets.copy_(torch.from_numpy(db))
            eager.poison()
            assert eager.enqueue(torch.cuda.current_stream(cuda_dev)) == 0
            torch.cuda.synchronize(cuda_dev)
            assert np.array_equal(eager.result(), wb)
        assert np.array_equal(replay(da), first), i


class _Segmented(object):
    """ryolo_rnms_segmented on ragged score-sorted sets, one of them a single box"""
    sizes = [1, 200, 64, 333, 65]

    def __init__(self, L, dev):
        self.L = L
        m = sum(self.sizes)
        self.dets = torch.zeros(m, 6, device=dev)
        self.off = torch.tensor(np.concatenate([[0], np.cumsum(self.sizes)]), dtype=torch.int32, device=dev)
        self.flags = torch.zeros(m, dtype=torch.uint8, device=dev)
        self.nbytes = L.lib().ryolo_rnms_segmented_workspace_bytes(m, len(self.sizes), max(self.sizes))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)

    def contents(self, which):
        sets = [riou.random_boxes(m, seed=40 + 100 * which + k, extent=60.0) for k, m in enumerate(self.sizes)]
        sets = [b[np.argsort(-b[:, 5], kind="stable")] for b in sets]
        want = []
        for b in sets:
            w = np.zeros(len(b), bool)
            w[riou.rnms(b, 0.3)] = True
            want.append(w)
        return np.concatenate(sets), np.concatenate(want)

    def load(self, inp):
        self.dets.copy_(torch.from_numpy(inp))
        self.flags.fill_(7)

    def enqueue(self, stream):
        return self.L.lib().ryolo_rnms_segmented(self.dets.data_ptr(), self.dets.size(0), 6, self.off.data_ptr(), len(self.sizes),
                                                 max(self.sizes), 0.3, self.flags.data_ptr(), self.ws.data_ptr(), self.nbytes,
                                                 stream.cuda_stream)

    def check(self, want):
        got = self.flags.cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), want)

    @staticmethod
    def differ(wa, wb):
        return not np.array_equal(wa, wb)


class _IouMatrix(object):
    """ryolo_riou_matrix (bit-exact vs oracle.riou) / ryolo_skew_iou_matrix (1e-6 vs oracle/poly_iou.py, include/ryolo.h)"""
    n1, n2 = 48, 40

    def __init__(self, L, dev, skew):
        self.L, self.skew = L, skew
        self.b1 = torch.zeros(self.n1, 5, device=dev)
        self.b2 = torch.zeros(self.n2, 5, device=dev)
        self.out = torch.zeros(self.n1, self.n2, device=dev)

    def contents(self, which):
        d1 = np.ascontiguousarray(riou.random_boxes(self.n1, seed=3 + 10 * which, extent=200.0)[:, :5])
        d2 = np.ascontiguousarray(riou.random_boxes(self.n2, seed=4 + 10 * which, extent=200.0)[:, :5])
        want = pi.skew_iou_matrix(d1, d2) if self.skew else riou.riou_matrix(d1, d2)
        assert (np.asarray(want) > 0.05).sum() > 20                      # the sets do overlap
        return (d1, d2), np.asarray(want)

    def load(self, inp):
        self.b1.copy_(torch.from_numpy(inp[0]))
        self.b2.copy_(torch.from_numpy(inp[1]))
        self.out.fill_(-3.0)

    def enqueue(self, stream):
        fn = self.L.lib().ryolo_skew_iou_matrix if self.skew else self.L.lib().ryolo_riou_matrix
        return fn(self.b1.data_ptr(), self.n1, 5, self.b2.data_ptr(), self.n2, 5, self.out.data_ptr(), stream.cuda_stream)

    def check(self, want):
        got = self.out.cpu().numpy()
        if self.skew:
            err = np.abs(got.astype(np.float64) - want).max()
            assert err <= 1e-6, err
        else:
            assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))

    @staticmethod
    def differ(wa, wb):
        return np.abs(np.asarray(wa, np.float64) - np.asarray(wb, np.float64)).max() > 0.1


class _DecodeFilter(object):
    """ryolo_yolo_decode_filter on a seeded head; reference and comparison of test_decode_filter_kernel_direct_vs_oracle
    (tests/test_model_gpu.py): oracle.darknet_oracle.decode + the filter half of non_max_suppression -- the same surviving rows, values
    to fp32 rounding of exp / sigmoid / atan; rows within 1e-4 of the score threshold may fall either way."""
    bs, ny, nx, na, nc, cf, thr, cap = 2, 5, 7, 6, 1, 1.0, 0.55, 4096

    def __init__(self, L, dev):
        self.L, self.no = L, self.nc + 6
        self.anchors = torch.tensor([[30., 10., -0.6], [30., 10., 0.6], [60., 20., -0.6], [60., 20., 0.6], [90., 30., -0.6], [90., 30., 0.6]])
        self.anchors_d = self.anchors.to(dev)
        self.cpad = (self.na * self.no + 7) // 8 * 8
        self.hd = torch.zeros(self.bs, self.ny, self.nx, self.cpad, dtype=torch.bfloat16, device=dev)
        self.cand = torch.zeros(self.cap, 8, device=dev)
        self.rows = torch.zeros(self.cap, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stride = float(max(self.ny, self.nx) * 16) / float(max(self.nx, self.ny))

    def contents(self, which):
        from oracle import darknet_oracle as do
        no, na = self.no, self.na
        g = torch.Generator().manual_seed(41 + 1000 * which)
        head = torch.randn(self.bs, na * no, self.ny, self.nx, generator=g) * 1.2
        head[:, 5::no] += 1.0                                   # some objectness above the threshold
        head = head.to(torch.bfloat16)
        io, _ = do.decode(head.float(), self.anchors.numpy(), (self.ny * 16, self.nx * 16), cf=self.cf, arc="default", nc=self.nc)
        cc, _ = io[..., 6:].max(2)
        score = io[..., 5] * cc
        keep = (score > self.thr) & (io[..., 2:4] > 2.0).all(2) & torch.isfinite(io).all(2)
        safe = (score - self.thr).abs() > 1e-4
        hd = torch.zeros(self.bs, self.ny, self.nx, self.cpad, dtype=torch.bfloat16)
        hd[..., :na * no] = head.permute(0, 2, 3, 1)
        return hd, (io, keep, safe)

    def load(self, inp):
        self.hd.copy_(inp)
        self.cand.fill_(-5.0)
        self.rows.fill_(-1)
        self.cnt.zero_()                                        # the caller's duty (include/ryolo.h), before every call / replay

    def enqueue(self, stream):
        total = self.na * self.ny * self.nx
        return self.L.lib().ryolo_yolo_decode_filter(self.hd.data_ptr(), self.hd.stride(2), self.bs, self.ny, self.nx, self.na, self.no,
                                                     self.anchors_d.data_ptr(), self.stride, self.cf, 0, self.thr, 2.0, total, 0,
                                                     self.cand.data_ptr(), self.rows.data_ptr(), self.cnt.data_ptr(), self.cap,
                                                     stream.cuda_stream)

    def check(self, want):
        io, keep, safe = want
        m = int(self.cnt.item())
        assert 0 < m <= self.cap
        rid, o = self.rows[:m].sort()
        got = self.cand[:m][o].cpu()
        rid = rid.cpu()
        want_ids = torch.nonzero(keep.flatten()).flatten()
        sure = set(torch.nonzero((keep & safe).flatten()).flatten().tolist())
        maybe = set(torch.nonzero((~safe).flatten()).flatten().tolist())
        got_ids = set(rid.tolist())
        assert len(got_ids) == m
        assert sure <= got_ids and got_ids <= (set(want_ids.tolist()) | maybe) and len(sure) > 20
        flat = io.reshape(-1, self.no)
        for r, row in zip(rid.tolist(), got):
            ref = flat[r]
            exp = torch.cat((ref[:5], (ref[5] * ref[6:].max()).view(1), ref[6:].max().view(1), ref[6:].argmax().float().view(1)))
            assert torch.allclose(row, exp, rtol=2e-5, atol=1e-5), (r, row, exp)

    @staticmethod
    def differ(wa, wb):
        ka, kb = (set(torch.nonzero((w[1] & w[2]).flatten()).flatten().tolist()) for w in (wa, wb))
        return len(ka ^ kb) > 20


@pytest.mark.parametrize("entry", ["rnms_segmented", "riou_matrix", "skew_iou_matrix", "yolo_decode_filter"])
def test_small_entry_points_captured_replay_on_new_contents(L, cuda_dev, entry):
    """The other entry points of the detection half, each captured on a side stream (after one eager warm-up call) and
    replayed on contents A, B, A written to the same pointers: each replay gives its contents' reference, and A's differs from B's."""
    op = {"rnms_segmented": lambda: _Segmented(L, cuda_dev), "riou_matrix": lambda: _IouMatrix(L, cuda_dev, False),
          "skew_iou_matrix": lambda: _IouMatrix(L, cuda_dev, True), "yolo_decode_filter": lambda: _DecodeFilter(L, cuda_dev)}[entry]()
    (ia, wa), (ib, wb) = op.contents(0), op.contents(1)
    assert op.differ(wa, wb)
    op.load(ia)
    assert op.enqueue(torch.cuda.current_stream(cuda_dev)) == 0
    torch.cuda.synchronize(cuda_dev)
    op.check(wa)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        rc = op.enqueue(torch.cuda.current_stream(cuda_dev))
    assert rc == 0, L.lib().ryolo_strerror(rc)
    for inp, want in ((ia, wa), (ib, wb), (ia, wa)):
        op.load(inp)
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        op.check(want)


# ------------------------------------------------------------------------------------------------ c / d(ii). two host threads
def _run_two_threads(workers, rounds, timeout):
    """workers: callables f(round) run by one thread each, all threads meeting at a barrier before every round so that their enqueues
    interleave.  A fixed number of rounds; the first exception of any thread is re-raised here; a thread still alive after `timeout`
    seconds is a failure, not a hang of the suite (daemon threads)."""
    barrier = threading.Barrier(len(workers))
    errors = []

    def body(i, f):
        try:
            for r in range(rounds):
                barrier.wait(timeout=timeout)
                f(r)
        except threading.BrokenBarrierError:
            errors.append((i, RuntimeError("thread %d: the other thread left the barrier (it failed or timed out)" % i), False))
        except BaseException as e:      # noqa: B902  (assertion errors included: they are re-raised in the main thread)
            errors.append((i, e, True))
            barrier.abort()

    threads = [threading.Thread(target=body, args=(i, f), daemon=True) for i, f in enumerate(workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    primary = [e for e in errors if e[2]] or errors
    if primary:
        raise primary[0][1]
    assert not alive, "threads %s did not finish within %d s" % (alive, timeout)


def test_rnms_two_host_threads_two_streams(L, cuda_dev):
    """Two host threads, each with its own stream, dets, keep, count and workspace: 26 000 clustered boxes against the oracle and the
    50 000-box golden workload against its committed SHA, four rounds with a barrier before each so that the two split calls are
    enqueued at the same time.  Both use the library's one second stream and its two events (serialised by the library's mutex;
    hipStreamWaitEvent binds to the record made at call time)."""
    da, wa = _case(*CASE_A)
    z = np.load(os.path.join(G, "rnms_keep_n50000.npz"))
    dg = riou.random_boxes(int(z["n"]), seed=int(z["seed"]))
    assert abs(float(z["thr"]) - 0.5) < 1e-12
    sha, nkeep = str(z["keep_sha256"]), len(z["keep"])
    calls = [NmsCall(L, len(da), cuda_dev), NmsCall(L, len(dg), cuda_dev)]
    calls[0].dets.copy_(torch.from_numpy(da))
    calls[1].dets.copy_(torch.from_numpy(dg))
    streams = [torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)]
    torch.cuda.synchronize(cuda_dev)
    lib = L.lib()

    def worker(i):
        c, s = calls[i], streams[i]
        thr = THR if i == 0 else 0.5

        def f(r):
            with torch.cuda.device(cuda_dev), torch.cuda.stream(s):
                c.poison()
                rc = lib.ryolo_rnms(c.dets.data_ptr(), c.n, 6, thr, c.keep.data_ptr(), c.cnt.data_ptr(), c.ws.data_ptr(), c.ws.numel(),
                                    s.cuda_stream)
                assert rc == 0, (i, r, lib.ryolo_strerror(rc))
                s.synchronize()
                got = c.result()
            if i == 0:
                assert np.array_equal(got, wa), (i, r)
            else:
                assert len(got) == nkeep, (i, r, len(got))
                assert hashlib.sha256(got.astype("<i8").tobytes()).hexdigest() == sha, (i, r)
        return f

    _run_two_threads([worker(0), worker(1)], rounds=4, timeout=180)


# ------------------------------------------------------------------------------------------------ d. the Python wrappers
def _sets(sizes, seed, extent):
    sets = [riou.random_boxes(m, seed=seed + k, extent=extent) for k, m in enumerate(sizes)]
    sets = [b[np.argsort(-b[:, 5], kind="stable")] for b in sets]
    want = []
    for b in sets:
        w = np.zeros(len(b), bool)
        w[riou.rnms(b, 0.3, nthreads=oracle.host_cores(8))] = True
        want.append(w)
    return np.concatenate(sets), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), np.concatenate(want)


def _dev_sets(sizes, seed, extent, dev):
    d, off, want = _sets(sizes, seed, extent)
    return torch.from_numpy(d).to(dev), torch.from_numpy(off).to(dev), max(sizes), want


def test_r_nms_segmented_on_two_streams_back_to_back(L, cuda_dev):
    """One host thread: r_nms_segmented on stream S1 with sets X and at once on S2 with sets Y of other sizes (a shared scratch tensor
    would be laid out differently by the two), no synchronisation between the calls: each flag vector = its sets' oracle."""
    from rotate_yolov3_amd.utils.nms.r_nms import r_nms_segmented
    x = _dev_sets([1, 1800, 1500, 2000, 1333, 1700, 1900, 65, 2000, 1600], 300, 250.0, cuda_dev)
    y = _dev_sets([700, 3, 640, 129, 900], 400, 120.0, cuda_dev)
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    with torch.cuda.stream(s1):
        fx = r_nms_segmented(x[0], x[1], x[2], 0.3)
    with torch.cuda.stream(s2):
        fy = r_nms_segmented(y[0], y[1], y[2], 0.3)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(fx.cpu().numpy().astype(bool), x[3])
    assert np.array_equal(fy.cpu().numpy().astype(bool), y[3])
    assert 0 < x[3].sum() < len(x[3]) and 0 < y[3].sum() < len(y[3])


def test_r_nms_from_two_host_threads(L, cuda_dev):
    """Two host threads calling r_nms (which synchronises its own stream) on streams of their own, 3 000 and 26 000 boxes, four rounds
    behind a barrier: every keep list = the oracle's."""
    from rotate_yolov3_amd.utils.nms.r_nms import r_nms
    ds = riou.random_boxes(3000, seed=9, extent=200.0)
    ws = riou.rnms(ds, THR)
    da, wa = _case(*CASE_A)
    dets = [torch.from_numpy(ds).to(cuda_dev), torch.from_numpy(da).to(cuda_dev)]
    wants = [ws, wa]
    streams = [torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)]
    torch.cuda.synchronize(cuda_dev)

    def worker(i):
        def f(r):
            with torch.cuda.device(cuda_dev), torch.cuda.stream(streams[i]):
                reps = 8 if i == 0 else 1                        # the short call several times per round: more overlap with the long one
                for _ in range(reps):
                    got = r_nms(dets[i], THR).cpu().numpy()
                    assert np.array_equal(got, wants[i]), (i, r)
        return f

    _run_two_threads([worker(0), worker(1)], rounds=4, timeout=180)


def test_scratch_request_on_another_stream_leaves_a_queued_call_alone(L, cuda_dev):
    """A call on S1 queued behind a long-running op (two 8192^2 fp32 matmuls) is still waiting when a call on S2 asks for more scratch
    than any call before it, and when the default stream then allocates and overwrites blocks of the first call's scratch size: the
    scratch of the queued call belongs to its stream until it has run -- S1's flags = the oracle's (and S2's too)."""
    from rotate_yolov3_amd.utils.nms.r_nms import r_nms_segmented
    x = _dev_sets([1, 200, 64, 333, 65, 1500], 500, 90.0, cuda_dev)
    y = _dev_sets([6000, 130], 600, 400.0, cuda_dev)
    nx = L.lib().ryolo_rnms_segmented_workspace_bytes(x[0].size(0), 6, x[2])
    ny = L.lib().ryolo_rnms_segmented_workspace_bytes(y[0].size(0), 2, y[2])
    assert ny > 1.25 * nx
    a = torch.randn(8192, 8192, device=cuda_dev)
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    with torch.cuda.stream(s1):
        b = a @ a
        b = b @ a
        fx = r_nms_segmented(x[0], x[1], x[2], 0.3)
    with torch.cuda.stream(s2):
        fy = r_nms_segmented(y[0], y[1], y[2], 0.3)
    junk = [torch.empty(nx, dtype=torch.uint8, device=cuda_dev).fill_(255) for _ in range(4)]
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize(cuda_dev)
    assert np.array_equal(fx.cpu().numpy().astype(bool), x[3])
    assert np.array_equal(fy.cpu().numpy().astype(bool), y[3])
    assert len(junk) == 4 and bool(torch.isfinite(b).any())


def test_r_nms_segmented_is_capturable(L, cuda_dev):
    """r_nms_segmented inside torch.cuda.graph(capture_error_mode="thread_local"), the way the eval engine captures its forward: the
    scratch comes from the graph's pool; replays on contents A, B, A written into the captured input give each one's oracle flags."""
    from rotate_yolov3_amd.utils.nms.r_nms import r_nms_segmented
    sizes = [1, 200, 64, 333, 65]
    da, off, wa = _sets(sizes, 40, 60.0)
    db, _, wb = _sets(sizes, 140, 60.0)
    assert not np.array_equal(wa, wb)
    dets = torch.from_numpy(da).to(cuda_dev)
    offd = torch.from_numpy(off).to(cuda_dev)
    assert np.array_equal(r_nms_segmented(dets, offd, max(sizes), 0.3).cpu().numpy().astype(bool), wa)      # eager warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(cuda_dev), capture_error_mode="thread_local"):
        flags = r_nms_segmented(dets, offd, max(sizes), 0.3)
    for d, want in ((da, wa), (db, wb), (da, wa)):
        dets.copy_(torch.from_numpy(d))
        g.replay()
        torch.cuda.synchronize(cuda_dev)
        assert np.array_equal(flags.cpu().numpy().astype(bool), want)
