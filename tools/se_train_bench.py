"""Training the se cfgs: the backward of the squeeze-and-excitation block (ryolo_se_bwd_nhwc, csrc/se_bwd.hip) per shape against the
streaming yardstick ryolo_add_nhwc and against ATen's backward of SELayer, and one training step of darknet53_se(512, 512) through the
ATen chain with se_backend 'torch' and 'hip'.

    python tools/se_train_bench.py [--bs 32] [--out profiles/se_training.txt]        call times + the step (profiler off)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/se_train_bench.py --trace-run      a run of its own: few plain launches,
                                                                                                  the per-kernel times come from the trace

Per-shape table: 76^2 x 256, 38^2 x 512 and 19^2 x 1024 at bs 32.  Call time as in tools/se_bench.py: `reps` calls captured in one
hipGraph, replayed until the timed window is >= 0.2 s, device events around the window; the contenders alternate in the same process,
median of the rounds with the spread:
    bwd    ryolo_se_bwd_nhwc with dx, dW1 and dW2 (four launches: x once, dy twice, dx once = 4 x the tensor); GB/s = 4 x tensor bytes / time
    add    ryolo_add_nhwc on the same tensor (three passes); GB/s = 3 x tensor bytes / time.  bwd/add = the ratio of the two bandwidths,
           i.e. (4/3 x add time) / bwd time: 1.0 = the backward streams its four passes as fast as add streams its three
    aten   torch.autograd.grad of SELayer's operator chain on fp32 NCHW CUDA tensors (x, fc.0.weight and fc.2.weight), the autograd graph
           built once; timed as eager calls (*): the autograd engine is not run inside a stream capture
The per-launch split is by difference between calls of the same ABI with outputs left out -- dx only (reduce, gate, apply), dW only
(reduce, gate, wgrad) -- so: wgrad = full - dx only, apply = full - dW only, reduce + gate = the rest; ryolo_se_nhwc (pool, gate, scale:
three passes) on the same x is printed beside them.

Step: forward + backward of sum_k <p_k, r_k> on darknet53_se(512, 512) in training mode, model.backend = 'torch', with se_backend
'torch' and 'hip' in the same process in alternating rounds (eager: autograd is not captured)."""
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
from rotate_yolov3_amd.model import hip_train_ops as T  # noqa: E402
from rotate_yolov3_amd.model.models import Darknet, SELayer  # noqa: E402
from tools.se_bench import SHAPES, graph_of, inputs  # noqa: E402


def window_us(run, reps, min_s=0.2):
    """us per call over a window of at least min_s seconds of run() (each = reps calls)"""
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
            return ms * 1e3 / (n * reps)
        n = max(n * 2, int(n * min_s * 1.2e3 / max(ms, 1e-3)))


def contenders(bs, h, w, c, dev):
    x, w1, w2 = inputs(bs, h, w, c, dev)
    g = torch.Generator(device="cpu").manual_seed(c + 1)
    dy = (torch.randn(bs, h, w, c, generator=g) + (torch.rand(bs, 1, 1, c, generator=g) * 4 - 2)).to(torch.bfloat16).to(dev)
    dx, y = torch.empty_like(x), torch.empty_like(x)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    ws = torch.empty(T.se_bwd_ws_bytes(bs, h, w, c, w1.shape[0]), dtype=torch.uint8, device=dev)
    ws_f = ops.se_workspace(bs, h, w, c, dev)
    L = _lib.lib()

    def add():
        _lib.check(L.ryolo_add_nhwc(x.data_ptr(), c, dy.data_ptr(), c, dx.data_ptr(), c, bs * h * w, c, _lib.stream_ptr(dev)), "ryolo_add_nhwc")

    se = SELayer(c).to(dev)
    with torch.no_grad():
        se.fc[0].weight.copy_(w1)
        se.fc[2].weight.copy_(w2)
    xa = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    dya = dy.float().permute(0, 3, 1, 2).contiguous()
    ya = se(xa)
    params = [xa, se.fc[0].weight, se.fc[2].weight]
    return dict(bwd=lambda: T.se_bwd_nhwc(x, dy, w1, w2, dx=dx, dw1=dw1, dw2=dw2, workspace=ws),
                bwd_dx=lambda: T.se_bwd_nhwc(x, dy, w1, w2, dx=dx, workspace=ws),
                bwd_dw=lambda: T.se_bwd_nhwc(x, dy, w1, w2, dw1=dw1, dw2=dw2, workspace=ws),
                fwd=lambda: ops.se_nhwc(x, w1, w2, out=y, workspace=ws_f),
                add=add,
                aten=lambda: torch.autograd.grad(ya, params, dya, retain_graph=True)), x


def runner(fn, reps):
    try:
        return graph_of(fn, reps).replay, ""
    except Exception:                                   # a backend that cannot be captured is timed as eager calls, and says so
        torch.cuda.synchronize()
        return (lambda: [fn() for _ in range(reps)]), "*"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-bs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help="few plain launches per shape, for a kernel trace taken in a run of its own")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "se_train_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    if a.trace_run:
        for (h, w, c) in SHAPES:
            fns, _ = contenders(a.bs, h, w, c, dev)
            for _ in range(10):
                fns["bwd"]()
                fns["add"]()
            torch.cuda.synchronize()
        return

    say("se_train_bench: bs %d, %s, library %s" % (a.bs, torch.cuda.get_device_name(0), _lib.lib().ryolo_build_id().decode()))
    say("call times in us: median of %d alternating rounds, each a >= 0.2 s window of graph replays (%d calls per graph; * = eager calls)"
        % (a.rounds, a.reps))
    say("GB/s: bwd = 4 x tensor bytes / time, add = 3 x tensor bytes / time; bwd/add = the ratio of the two (1.0: four passes at add's rate)")
    names = ("bwd", "add", "aten", "bwd_dx", "bwd_dw", "fwd")
    say("%-14s %9s | %9s %8s %9s %8s %8s | %10s %8s | %12s %8s %8s %9s | spread %%"
        % ("shape", "tensor MB", "bwd us", "bwd GB/s", "add us", "add GB/s", "bwd/add", "aten us", "aten/bwd", "reduce+gate", "wgrad", "apply",
           "(fwd us)"))
    for (h, w, c) in SHAPES:
        fns, x = contenders(a.bs, h, w, c, dev)
        run = {k: runner(fns[k], a.reps) for k in names if k != "aten"}
        run["aten"] = ((lambda fn=fns["aten"]: [fn() for _ in range(a.reps)]), "*")      # autograd is not captured: eager calls
        run["aten"][0]()                                                                  # (warm-up, as graph_of gives the others)
        torch.cuda.synchronize()
        t = {k: [] for k in names}
        for _ in range(a.rounds):
            for k in names:
                t[k].append(window_us(run[k][0], a.reps))
        m = {k: statistics.median(t[k]) for k in names}
        nbytes = 2.0 * x.numel()
        bw_bwd, bw_add = 4 * nbytes / m["bwd"] * 1e-3, 3 * nbytes / m["add"] * 1e-3
        wgrad, apply_ = m["bwd"] - m["bwd_dx"], m["bwd"] - m["bwd_dw"]
        say("%-14s %9.1f | %9.1f %8.0f %9.1f %8.0f %8.3f | %9.1f%s %8.2f | %12.1f %8.1f %8.1f %9.1f | %s"
            % ("%dx%dx%d" % (h, w, c), nbytes / 1e6, m["bwd"], bw_bwd, m["add"], bw_add, bw_bwd / bw_add, m["aten"], run["aten"][1] or " ",
               m["aten"] / m["bwd"], m["bwd"] - wgrad - apply_, wgrad, apply_, m["fwd"],
               " ".join("%.1f" % (50.0 * (max(t[k]) - min(t[k])) / m[k]) for k in names)))
        del run, fns
        flush()

    if not a.skip_step:
        say()
        say("training step (forward + backward) of darknet53_se(512, 512), bs %d, model.backend = 'torch', eager:" % a.step_bs)
        torch.manual_seed(0)
        model = Darknet(make_cfg.darknet53_se(512, 512), {"context_factor": 1.0}).train().to(dev)
        model.backend = "torch"
        x = torch.rand(a.step_bs, 3, 512, 512, device=dev)
        rs = None

        def step():
            nonlocal rs
            ps = model(x)
            if rs is None:
                g = torch.Generator(device=dev).manual_seed(1)
                rs = [torch.randn(p.shape, generator=g, device=dev) for p in ps]
            model.zero_grad(set_to_none=True)
            sum((p * r).sum() for p, r in zip(ps, rs)).backward()

        t = {"torch": [], "hip": []}
        for backend in ("torch", "hip"):
            model.se_backend = backend
            for _ in range(2):
                step()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for backend in ("torch", "hip"):
                model.se_backend = backend
                t[backend].append(window_us(step, 1, min_s=1.0) / 1e3)
        med = statistics.median
        for backend in ("torch", "hip"):
            say("se_backend = %-7s %9.2f ms per step (+-%.1f %%)"
                % (repr(backend), med(t[backend]), 50.0 * (max(t[backend]) - min(t[backend])) / med(t[backend])))
        say("'hip' / 'torch' = %.3f" % (med(t["hip"]) / med(t["torch"])))
    flush()


if __name__ == "__main__":
    main()
