"""Training the matrix cfgs: the dilated data gradient (ryolo_conv2d_dilated_dgrad, csrc/conv_dil.hip) and weight gradient
(ryolo_conv2d_dilated_wgrad, csrc/wgrad_dil.hip) per shape against ATen and against the library's own undilated gradients, and one
training step of darknet53_matrix(512, 512) through the ATen chain with shared_conv_backend 'torch' and 'hip'.

    python tools/matrix_train_bench.py [--out profiles/matrix_training.txt]

Per-shape table: the three dilated shapes of the 512^2 cfg (16^2 512->1024, 32^2 256->512, 64^2 128->256) x dilations (1,2) and (8,1) at
bs 1 and bs 32.  Call time as in tools/matrix_bench.py: `reps` calls captured in one hipGraph, replayed until the window is >= 0.2 s,
device events around the window; the contenders alternate in the same process, median of the rounds with the spread:
    dil    ryolo_conv2d_dilated_dgrad / ryolo_conv2d_dilated_wgrad (tile kernel + split-K reduce)
    plain  ryolo_conv2d_dgrad / ryolo_conv2d_wgrad on the same tensors, undilated, auto dispatch: the same flops through the tuned kernels
    aten   torch.ops.aten.convolution_backward on bf16 channels_last tensors with the same dilation, one output at a time
TFLOP/s = 2 * 9 * Cin * Cout * N*H*W / time (algorithmic).

Step: forward + backward of sum_k <p_k, r_k> on darknet53_matrix(512, 512) in training mode, model.backend = 'torch', with
shared_conv_backend 'torch' and 'hip' in the same process in alternating rounds (eager: autograd is not captured)."""
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
from rotate_yolov3_amd.model.models import Darknet  # noqa: E402
from tools.matrix_bench import DILS, SHAPES, graph_of, window_us  # noqa: E402


def contenders(bs, hw, cin, cout, dil, dev):
    g = torch.Generator().manual_seed(hw + cin)
    x = torch.randn(bs, hw, hw, cin, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.randn(bs, hw, hw, cout, generator=g).to(torch.bfloat16).to(dev)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dev)
    packed = T.pack_weights_dgrad(wt, 1)
    ones, zeros = torch.ones(ops.cpad(cin), device=dev), torch.zeros(ops.cpad(cin), device=dev)
    dx = torch.empty(bs, hw, hw, cin, dtype=torch.bfloat16, device=dev)
    dw = torch.empty(cout, cin, 3, 3, dtype=torch.float32, device=dev)
    d = T.dilated_desc(bs, hw, hw, cin, cout)
    ws_d = torch.empty(T.conv_dilated_wgrad_ws_bytes(d, dil), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(T.wgrad_ws_bytes(d), dtype=torch.uint8, device=dev)
    xa, dya = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)       # NCHW views of the NHWC tensors = channels_last
    wa = wt.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def aten(mask):
        return lambda: torch.ops.aten.convolution_backward(dya, xa, wa, None, [1, 1], list(dil), list(dil), False, [0, 0], 1, mask)
    return dict(dil_dgrad=lambda: T.conv_dilated_dgrad(d, dil, dy, packed, ones, zeros, dx),
                dil_wgrad=lambda: T.conv_dilated_wgrad(d, dil, x, dy, dw, False, ws_d),
                plain_dgrad=lambda: T.conv_dgrad(d, dy, packed, ones, zeros, dx, False),
                plain_wgrad=lambda: T.conv_wgrad(d, x, dy, cin, dw, False, ws_p),
                aten_dgrad=aten([True, False, False]), aten_wgrad=aten([False, True, False]))


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-bs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "matrix_train_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say("matrix_train_bench: %s, library %s" % (torch.cuda.get_device_name(0), _lib.lib().ryolo_build_id().decode()))
    say("call times in us: median of %d alternating rounds, each a >= 0.2 s window of graph replays (%d calls per graph; * = eager calls)"
        % (a.rounds, a.reps))
    names = ("dil_dgrad", "plain_dgrad", "aten_dgrad", "dil_wgrad", "plain_wgrad", "aten_wgrad")
    say("%-22s %-5s | %9s %7s %9s %7s %9s %7s | %9s %7s %9s %7s %9s %7s | spread %%"
        % ("shape", "dil", "dgrad dil", "TFLOP/s", "plain", "dil/pl", "aten", "dil/at", "wgrad dil", "TFLOP/s", "plain", "dil/pl", "aten", "dil/at"))
    for bs in (1, a.bs):
        for (hw, cin, cout) in SHAPES:
            for dil in DILS:
                fns = contenders(bs, hw, cin, cout, dil, dev)
                run = {k: runner(fns[k], a.reps) for k in names}
                t = {k: [] for k in names}
                for _ in range(a.rounds):
                    for k in names:
                        t[k].append(window_us(run[k][0], a.reps))
                m = {k: statistics.median(t[k]) for k in names}
                flops = 2.0 * 9 * cin * cout * bs * hw * hw
                say("%-22s %-5s | %9.1f %7.1f %9.1f %7.2f %8.1f%s %7.2f | %9.1f %7.1f %9.1f %7.2f %8.1f%s %7.2f | %s"
                    % ("bs%d %dx%d %d->%d" % (bs, hw, hw, cin, cout), "%dx%d" % dil,
                       m["dil_dgrad"], flops / m["dil_dgrad"] * 1e-6, m["plain_dgrad"], m["dil_dgrad"] / m["plain_dgrad"],
                       m["aten_dgrad"], run["aten_dgrad"][1] or " ", m["dil_dgrad"] / m["aten_dgrad"],
                       m["dil_wgrad"], flops / m["dil_wgrad"] * 1e-6, m["plain_wgrad"], m["dil_wgrad"] / m["plain_wgrad"],
                       m["aten_wgrad"], run["aten_wgrad"][1] or " ", m["dil_wgrad"] / m["aten_wgrad"],
                       " ".join("%.1f" % (50.0 * (max(t[k]) - min(t[k])) / m[k]) for k in names)))
                del run, fns
                flush()

    if not a.skip_step:
        say()
        say("training step (forward + backward) of darknet53_matrix(512, 512), bs %d, model.backend = 'torch', eager:" % a.step_bs)
        torch.manual_seed(0)
        model = Darknet(make_cfg.darknet53_matrix(512, 512), {"context_factor": 1.0}).train().to(dev)
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
            model.shared_conv_backend = backend
            for _ in range(2):
                step()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for backend in ("torch", "hip"):
                model.shared_conv_backend = backend
                t[backend].append(window_us(step, 1, min_s=1.0) / 1e3)
        med = statistics.median
        for backend in ("torch", "hip"):
            say("shared_conv_backend = %-7s %9.2f ms per step (+-%.1f %%), peak memory %.1f GB"
                % (repr(backend), med(t[backend]), 50.0 * (max(t[backend]) - min(t[backend])) / med(t[backend]),
                   torch.cuda.max_memory_allocated() / 1e9))
        say("'hip' / 'torch' = %.3f" % (med(t["hip"]) / med(t["torch"])))
    flush()


if __name__ == "__main__":
    main()
