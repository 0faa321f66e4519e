"""What does one optimizer step over Darknet-53's parameter tensors cost?  No engine, no forward: the parameter tensors of
Darknet(make_cfg.darknet53(608, 608)) on the GPU, seeded random gradients (shared by all contestants), the two param groups of
train.make_optimizer.  Contestants: torch.optim.Adam with defaults (what `--adam` ran before FusedAdam; the yardstick), torch.optim.Adam(fused=True)
if this build constructs it, FusedAdam with its per-tensor grid and with a grid capped near 2048 workgroups, and FusedSGD for scale.
    python tools/optim_step_bench.py                  ten interleaved rounds of 50 steps (order reversed on odd rounds), device events
    rocprofv3 --kernel-trace --stats -- python tools/optim_step_bench.py --steps 5
                                                      no timing: every contestant runs exactly 5 steps, so a kernel's calls / 5 in the stats are
                                                      its launches per step (adam_batch_kernel: FusedAdam, both grids; sgd_batch_kernel: FusedSGD;
                                                      FusedAdamMathFunctor: torch's fused=True; every other kernel: torch.optim.Adam's foreach chain)"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import rotate_yolov3_amd  # noqa: E402,F401

COPY_TBS, PEAK_TBS = 6.29, 8.0       # measured float4 copy rate and the HBM3E specification of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0, help="no timing: run every contestant exactly this many steps (for a kernel trace)")
    ap.add_argument("--size", type=int, default=608)
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.utils.fused_adam import FusedAdam
    from rotate_yolov3_amd.utils.fused_sgd import FusedSGD
    from train import make_optimizer
    dev = torch.device("cuda:0")
    hyp = {"context_factor": 1.0, "lr0": 1e-4, "momentum": 0.97, "weight_decay": 0.0004569}
    torch.manual_seed(0)
    base = Darknet(make_cfg.darknet53(a.size, a.size), hyp).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in base.parameters()]
    nparam = sum(p.numel() for p in base.parameters())
    need = 7 * 4 * nparam            # read p, g, m, v; write p, m, v

    def contestant(build):
        m = copy.deepcopy(base)
        opt = build(m)
        for p, g in zip(m.parameters(), grads):
            p.grad = g
        return opt

    def torch_fused(m):
        groups = make_optimizer(m, hyp, adam=True, fused=False).param_groups
        return torch.optim.Adam([{"params": g["params"], "weight_decay": g["weight_decay"]} for g in groups], lr=hyp["lr0"], fused=True)

    def fused_adam(m):                       # built by hand: make_optimizer picks it only if it won here
        groups = make_optimizer(m, hyp, adam=True, fused=False).param_groups
        opt = FusedAdam(groups[0]["params"], lr=hyp["lr0"])
        opt.add_param_group({"params": groups[1]["params"], "weight_decay": groups[1]["weight_decay"]})
        return opt

    def capped(m):
        opt = fused_adam(m)
        opt.elems_per_block = 32768          # ceil(n / 32768) workgroups per tensor instead of ceil(n / 2048): about 2000 in all
        return opt

    entries = [("torch.optim.Adam (defaults)", lambda m: make_optimizer(m, hyp, adam=True, fused=False)),
               ("torch.optim.Adam(fused=True)", torch_fused),
               ("FusedAdam", fused_adam),
               ("FusedAdam, grid capped", capped),
               ("FusedSGD", lambda m: make_optimizer(m, hyp))]
    opts = []
    for name, build in entries:
        try:
            opts.append((name, contestant(build)))
        except Exception as e:       # only torch's fused=True may be missing from a build
            if "fused=True" not in name:
                raise
            print("%s: not constructed by this build (%s)" % (name, str(e).splitlines()[0][:100]))
    assert isinstance(dict(opts)["FusedSGD"], FusedSGD)
    print("Darknet-53 %dx%d: %d parameter tensors, %d elements, two param groups (weight decay on Conv2d.weight)"
          % (a.size, a.size, len(grads), nparam))
    if a.steps:
        for name, opt in opts:
            for _ in range(a.steps):
                opt.step()
            torch.cuda.synchronize()
            blocks = " (%d workgroups)" % opt._blocks if isinstance(opt, FusedAdam) else ""
            print("%-32s %d steps%s" % (name, a.steps, blocks))
        return
    for name, opt in opts:
        for _ in range(a.warmup):
            opt.step()
    torch.cuda.synchronize()
    times = dict((name, []) for name, _ in opts)
    for r in range(a.rounds):
        for name, opt in (opts if r % 2 == 0 else opts[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.per_round):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.per_round)
    print("%d interleaved rounds of %d steps after %d warm-up steps, order reversed on odd rounds; ms per step between two device events "
          "(back-to-back steps: the larger of the host's and the device's time)" % (a.rounds, a.per_round, a.warmup))
    print("%-32s %9s %9s %9s   %s" % ("contestant", "median", "min", "max", "rounds"))
    for name, _ in opts:
        t = times[name]
        print("%-32s %9.3f %9.3f %9.3f   %s" % (name, statistics.median(t), min(t), max(t), " ".join("%.3f" % v for v in t)))
    print("bytes the algorithm needs (read p, g, m, v; write p, m, v): 7 x 4 x %d = %.1f MB -> %.3f ms at %.2f TB/s (float4 copy), %.3f ms at "
          "%.1f TB/s (peak)" % (nparam, need / 1e6, need / COPY_TBS / 1e9, COPY_TBS, need / PEAK_TBS / 1e9, PEAK_TBS))
    for name in ("FusedAdam", "FusedAdam, grid capped"):
        med = statistics.median(times[name])
        print("%-32s %.2f TB/s = %.0f %% of the copy rate, %.0f %% of the peak" % (name, need / med / 1e9, 100 * need / med / 1e9 / COPY_TBS,
                                                                                  100 * need / med / 1e9 / PEAK_TBS))
    ref = times["torch.optim.Adam (defaults)"]
    for name in ("FusedAdam", "FusedAdam, grid capped"):
        wins = sum(f < t for f, t in zip(times[name], ref))
        print("%s faster than torch.optim.Adam (defaults) in %d of %d rounds, x%.2f at the medians"
              % (name, wins, a.rounds, statistics.median(ref) / statistics.median(times[name])))


if __name__ == "__main__":
    main()
