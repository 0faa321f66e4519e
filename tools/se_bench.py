"""Squeeze-and-excitation on the HIP inference path: ryolo_se_nhwc against the streaming yardstick ryolo_add_nhwc, and the replayed
eval forward of darknet53_se() against darknet53().

    python tools/se_bench.py [--bs 32] [--out profiles/se_inference.txt]        call times + forwards (profiler off)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/se_bench.py --trace-run      a run of its own: few plain launches,
                                                                                            the per-kernel times come from the trace

Call time: `reps` calls captured in one hipGraph (a Python / ctypes call costs more than the short shapes take), the graph replayed
until the timed window is >= 0.2 s, device events around the window; se and add alternate, five rounds, the median is reported with
the spread.  Effective bandwidth = 3 x tensor bytes / time for both calls (se reads x twice and writes y; add reads a, b and writes y).
Target (76^2 and 38^2 shapes): se bandwidth >= 0.9 x add bandwidth in the same run; 19^2 (23 MB, launch-bound) is reported without a bar."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.cfg import make_cfg  # noqa: E402
from rotate_yolov3_amd.model import hip_ops as ops  # noqa: E402
from rotate_yolov3_amd.model.engine import HipEngine  # noqa: E402
from rotate_yolov3_amd.model.models import Darknet  # noqa: E402

SHAPES = [(76, 76, 256), (38, 38, 512), (19, 19, 1024)]


def graph_of(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def window_us(g, reps, min_s=0.2):
    """us per call over a window of at least min_s seconds of replays"""
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_s * 1e3:
            return ms * 1e3 / (n * reps)
        n = max(n * 2, int(n * min_s * 1.2e3 / max(ms, 1e-3)))


def inputs(bs, h, w, c, dev):
    g = torch.Generator(device="cpu").manual_seed(c)
    x = (torch.randn(bs, h, w, c, generator=g) + (torch.rand(bs, 1, 1, c, generator=g) * 4 - 2)).to(torch.bfloat16).to(dev)
    hid = c // 16
    w1 = ((torch.rand(hid, c, generator=g) * 2 - 1) * (3.0 / c) ** 0.5).to(dev)
    w2 = (2 * (torch.rand(c, hid, generator=g) * 2 - 1) * (3.0 / hid) ** 0.5).to(dev)
    return x, w1, w2


def se_and_add(bs, h, w, c, dev):
    x, w1, w2 = inputs(bs, h, w, c, dev)
    b = x.flip(0).contiguous()
    y = torch.empty_like(x)
    ws = ops.se_workspace(bs, h, w, c, dev)
    L = _lib.lib()

    def se():
        ops.se_nhwc(x, w1, w2, out=y, workspace=ws)

    def add():
        _lib.check(L.ryolo_add_nhwc(x.data_ptr(), c, b.data_ptr(), c, y.data_ptr(), c, bs * h * w, c, _lib.stream_ptr(dev)), "ryolo_add_nhwc")
    return se, add, x


def replayed_engine(cfg, bs, dev):
    m = Darknet(cfg, {"context_factor": 1.0}).eval().to(dev)
    x = torch.rand(bs, 3, 608, 608, device=dev)
    eng = HipEngine(m, x.shape, dev, use_graph=True, want_p=False)
    with torch.no_grad():
        for _ in range(3):
            eng(x)
    torch.cuda.synchronize()
    return eng, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="few plain launches per shape, for a kernel trace taken in a run of its own")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "se_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.trace_run:
        for (h, w, c) in SHAPES:
            se, add, _ = se_and_add(a.bs, h, w, c, dev)
            for _ in range(10):
                se()
                add()
            torch.cuda.synchronize()
        return

    say("se_bench: bs %d, %s, library %s" % (a.bs, torch.cuda.get_device_name(0), _lib.lib().ryolo_build_id().decode()))
    say("call times: median of %d alternating rounds, each a >= 0.2 s window of graph replays (%d calls per graph); GB/s = 3 x tensor bytes / time"
        % (a.rounds, a.reps))
    say("%-14s %9s %10s %9s %10s %8s %8s  %s" % ("shape", "tensor MB", "se us", "se GB/s", "add us", "add GB/s", "se/add", "spread se / add"))
    for (h, w, c) in SHAPES:
        se, add, x = se_and_add(a.bs, h, w, c, dev)
        gs, ga = graph_of(se, a.reps), graph_of(add, a.reps)
        ts, ta = [], []
        for _ in range(a.rounds):
            ts.append(window_us(gs, a.reps))
            ta.append(window_us(ga, a.reps))
        t_se, t_add = statistics.median(ts), statistics.median(ta)
        nbytes = 2.0 * x.numel()
        bw_se, bw_add = 3 * nbytes / t_se * 1e-3, 3 * nbytes / t_add * 1e-3
        ratio = bw_se / bw_add
        verdict = "" if h == 19 else ("  target 0.9 met" if ratio >= 0.9 else "  target 0.9 MISSED")
        say("%-14s %9.1f %10.1f %9.0f %10.1f %8.0f %8.3f  +-%.1f %% / +-%.1f %%%s"
            % ("%dx%dx%d" % (h, w, c), nbytes / 1e6, t_se, bw_se, t_add, bw_add, ratio,
               50.0 * (max(ts) - min(ts)) / t_se, 50.0 * (max(ta) - min(ta)) / t_add, verdict))
        del gs, ga

    say()
    say("replayed eval forward (hipGraph, want_p off), 608^2 bs %d: median of %d alternating rounds of >= 0.2 s" % (a.bs, a.rounds))
    e_se, x_se = replayed_engine(make_cfg.darknet53_se(), a.bs, dev)
    e_pl, x_pl = replayed_engine(make_cfg.darknet53(), a.bs, dev)
    t_se, t_pl = [], []
    for _ in range(a.rounds):
        t_se.append(window_us(e_se.graph, 1) / 1e3)
        t_pl.append(window_us(e_pl.graph, 1) / 1e3)
    m_se, m_pl = statistics.median(t_se), statistics.median(t_pl)
    se_bytes = sum(i["bytes"] for i in e_se.op_info if i["name"] == "se_nhwc")
    say("darknet53_se  %.3f ms (+-%.1f %%)   darknet53  %.3f ms (+-%.1f %%)   added by 20 se layers: %.3f ms for %.0f MB of se traffic (%.0f GB/s)"
        % (m_se, 50.0 * (max(t_se) - min(t_se)) / m_se, m_pl, 50.0 * (max(t_pl) - min(t_pl)) / m_pl, m_se - m_pl, se_bytes / 1e6,
           se_bytes / max(m_se - m_pl, 1e-9) * 1e-6))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
