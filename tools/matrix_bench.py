"""The matrix cfgs on the HIP inference path: ryolo_conv2d_dilated (csrc/conv_dil.hip) per shape against the library's own undilated 3x3
and against ATen, and the eval forward of darknet53_matrix(512, 512).

    python tools/matrix_bench.py [--out profiles/matrix_inference.txt]

Per-shape table: the six dilated shapes of the 512^2 cfg (16^2 512->1024, 32^2 256->512, 64^2 128->256; bs 1 and bs 32), dilations (1,2)
and (8,1).  Call time: `reps` calls captured in one hipGraph (a ctypes call costs more than the bs-1 shapes take), replayed until the
window is >= 0.2 s, device events around the window; the contenders alternate in the same process, median of the rounds with the spread:
    dil    ryolo_conv2d_dilated
    plain  ryolo_conv2d_bn_act on the same tensors, undilated, auto dispatch: the same flops and bytes through the tuned kernels
    aten   F.conv2d(x, w, padding=dil, dilation=dil), bf16, channels_last
TFLOP/s = 2 * 9 * Cin * Cout * N*H*W / time (algorithmic); share of peak = the least time the hardware could take -- the larger of flops
over the bf16 MFMA peak and algorithmic bytes (x + w + y) over the HBM peak -- over the measured time, with the bound that applies.

Forward: darknet53_matrix(512, 512) at bs 32, want_p off: eager launches against graph replay, with and without the aliasing of repeated
shared layers (RYOLO_SHARED_ALIAS=0), and the ATen chain (model.backend = 'torch', fp32, eval) on the same input."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd import _lib  # noqa: E402
from rotate_yolov3_amd.cfg import make_cfg  # noqa: E402
from rotate_yolov3_amd.model import hip_ops as ops  # noqa: E402
from rotate_yolov3_amd.model.engine import HipEngine  # noqa: E402
from rotate_yolov3_amd.model.models import Darknet  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0      # bf16 dense
HBM_PEAK_TBS = 8.0
SHAPES = [(16, 512, 1024), (32, 256, 512), (64, 128, 256)]      # (map, C_in, C_out) of the three levels at 512^2
DILS = [(1, 2), (8, 1)]


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


def window_us(run, per, min_s=0.2):
    """us per call over a window of at least min_s seconds of run() (which makes `per` calls)"""
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_s * 1e3:
            return ms * 1e3 / (n * per)
        n = max(n * 2, int(n * min_s * 1.2e3 / max(ms, 1e-3)))


def contenders(bs, hw, cin, cout, dil, dev):
    g = torch.Generator().manual_seed(hw + cin)
    x = torch.randn(bs, hw, hw, cin, generator=g).to(torch.bfloat16).to(dev)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dev)
    packed = ops.pack_weights(wt, cin_pad=cin)
    sc, sh = torch.ones(ops.cpad(cout), device=dev), torch.zeros(ops.cpad(cout), device=dev)
    y = torch.empty(bs, hw, hw, cout, dtype=torch.bfloat16, device=dev)
    xa = x.permute(0, 3, 1, 2)                                   # NCHW view of the NHWC tensor = channels_last
    wa = wt.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def dil_fn():
        ops.conv2d_dilated(x, packed, sc, sh, cout, dil, out=y)

    def plain_fn():
        ops.conv2d_bn_act(x, packed, sc, sh, cout, 3, stride=1, pad=1, act=ops.ACT_LINEAR, out=y)

    def aten_fn():
        F.conv2d(xa, wa, None, 1, dil, dil)
    name = ops.conv_kernel_name(bs, hw, hw, cin, cout, 3)
    return dil_fn, plain_fn, aten_fn, name


def timed_engine(m, x, dev, use_graph):
    eng = HipEngine(m, x.shape, dev, use_graph=use_graph, want_p=False)
    with torch.no_grad():
        for _ in range(3):
            eng(x)
    torch.cuda.synchronize()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-forward", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "matrix_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say("matrix_bench: %s, library %s" % (torch.cuda.get_device_name(0), _lib.lib().ryolo_build_id().decode()))
    say("call times: median of %d alternating rounds, each a >= 0.2 s window of graph replays (%d calls per graph)" % (a.rounds, a.reps))
    say("%-22s %-6s %9s %8s %7s %-6s | %9s %7s %-26s | %9s %7s" % ("shape", "dil", "dil us", "TFLOP/s", "of peak", "bound", "plain us",
                                                                 "dil/pl", "plain kernel", "aten us", "dil/at"))
    for bs in (1, a.bs):
        for (hw, cin, cout) in SHAPES:
            for dil in DILS:
                fd, fp, fa, pname = contenders(bs, hw, cin, cout, dil, dev)
                gd, gp = graph_of(fd, a.reps), graph_of(fp, a.reps)
                try:
                    ga = graph_of(fa, a.reps)
                    run_a, aten_how = ga.replay, ""
                except Exception:                               # a backend that cannot be captured is timed as eager calls, and says so
                    torch.cuda.synchronize()
                    run_a, aten_how = (lambda: [fa() for _ in range(a.reps)]), " (eager)"
                td, tp, ta = [], [], []
                for _ in range(a.rounds):
                    td.append(window_us(gd.replay, a.reps))
                    tp.append(window_us(gp.replay, a.reps))
                    ta.append(window_us(run_a, a.reps))
                md, mp, ma = statistics.median(td), statistics.median(tp), statistics.median(ta)
                flops = 2.0 * 9 * cin * cout * bs * hw * hw
                nbytes = 2.0 * (bs * hw * hw * (cin + cout) + 9 * cin * cout)
                t_mfma, t_hbm = flops / (MFMA_PEAK_TFLOPS * 1e12) * 1e6, nbytes / (HBM_PEAK_TBS * 1e12) * 1e6
                say("%-22s %-6s %9.1f %8.1f %6.1f%% %-6s | %9.1f %7.2f %-26s | %9.1f %7.2f%s   spread +-%.1f / %.1f / %.1f %%"
                    % ("bs%d %dx%d %d->%d" % (bs, hw, hw, cin, cout), "%dx%d" % dil, md, flops / md * 1e-6, 100.0 * max(t_mfma, t_hbm) / md,
                       "mfma" if t_mfma >= t_hbm else "hbm", mp, md / mp, pname, ma, md / ma, aten_how,
                       50.0 * (max(td) - min(td)) / md, 50.0 * (max(tp) - min(tp)) / mp, 50.0 * (max(ta) - min(ta)) / ma))
                del gd, gp
                flush()

    if not a.skip_forward:
        say()
        say("eval forward of darknet53_matrix(512, 512), bs %d, want_p off: median of %d alternating rounds of >= 0.2 s" % (a.bs, a.rounds))
        m = Darknet(make_cfg.darknet53_matrix(512, 512), {"context_factor": 1.0}).eval().to(dev)
        x = torch.rand(a.bs, 3, 512, 512, device=dev)
        e_eager, e_graph = timed_engine(m, x, dev, False), timed_engine(m, x, dev, True)
        os.environ["RYOLO_SHARED_ALIAS"] = "0"
        e_noalias = timed_engine(m, x, dev, True)
        del os.environ["RYOLO_SHARED_ALIAS"]
        m.backend = "torch"
        with torch.no_grad():
            for _ in range(2):
                m(x)
        torch.cuda.synchronize()
        te, tg, tn, tt = [], [], [], []
        with torch.no_grad():
            for _ in range(a.rounds):
                te.append(window_us(lambda: e_eager(x), 1) / 1e3)
                tg.append(window_us(e_graph.graph.replay, 1) / 1e3)
                tn.append(window_us(e_noalias.graph.replay, 1) / 1e3)
                tt.append(window_us(lambda: m(x), 1, min_s=0.5) / 1e3)
        med = statistics.median
        dil_flops = sum(i["flops"] for i in e_graph.op_info if i["name"].startswith("conv_dil<"))
        all_flops = sum(i["flops"] for i in e_graph.op_info)
        say("launches per forward: %d (%d dilated, %d aliased shared layers not launched; %d without aliasing)"
            % (len(e_graph.ops), sum(i["name"].startswith("conv_dil<") for i in e_graph.op_info), len(e_noalias.ops) - len(e_graph.ops), len(e_noalias.ops)))
        say("algorithmic GFLOP per forward: %.1f, of which dilated convs %.1f" % (all_flops / 1e9, dil_flops / 1e9))
        say("HIP eager        %8.3f ms (+-%.1f %%)" % (med(te), 50.0 * (max(te) - min(te)) / med(te)))
        say("HIP graph replay %8.3f ms (+-%.1f %%)   %.1f TFLOP/s whole-forward rate (not a kernel's share of peak)"
            % (med(tg), 50.0 * (max(tg) - min(tg)) / med(tg), all_flops / med(tg) * 1e-9))
        say("  without aliasing %6.3f ms (+-%.1f %%)   aliasing saves %.3f ms" % (med(tn), 50.0 * (max(tn) - min(tn)) / med(tn), med(tn) - med(tg)))
        say("ATen chain (backend='torch', fp32) %8.3f ms (+-%.1f %%)   HIP graph replay is %.1f x faster"
            % (med(tt), 50.0 * (max(tt) - min(tt)) / med(tt), med(tt) / med(tg)))
    flush()


if __name__ == "__main__":
    main()
