"""What does freezing layers buy on the HIP TrainEngine?  One optimizer step end to end -- forward, fused loss, backward, FusedSGD -- of
bench.py's training step (Darknet-53, its hyp, the 'default' arc, its seeded weights, input and targets; bs 64 at 608^2) under four
requires_grad patterns:

    all        every parameter trains (the step bench.py times)
    transfer   train.py --transfer: weight and bias of the convs in front of the yolo layers
    prebias    train.py --prebias: their biases
    trunk      layers < 75 frozen: the three FPN heads train

    python tools/freeze_step_bench.py [--out profiles/freeze_step.txt]

Times: one model per pattern (each keeps its own engine) in ONE process, `--rounds` interleaved rounds of `--per-round` steps, the order
reversed on odd rounds, ms per step between two device events, after a warm-up past the graph capture (two eager steps, then the capture).
Memory and launches: each pattern once more in a fresh child process (`--child NAME`): torch.cuda.max_memory_allocated after the same
warm-up, and the C ABI launch calls of one eagerly launched backward (ryolo_* calls of TrainEngine._backward_launch; the captured graphs
replay exactly these).  The ratio of every pattern is taken against `all` of the same run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERNS = ("all", "transfer", "prebias", "trunk")
HYP = {"giou": 0.1, "cls": 27.76, "cls_pw": 1.0, "obj": 20.35, "obj_pw": 1.0, "iou_t": 0.5, "ang_t": 3.1415926 / 12,
       "reg": 1.0, "fl_gamma": 0.5, "context_factor": 1.0, "lr0": 1e-4, "momentum": 0.97, "weight_decay": 0.0004569}     # bench.py bench_train


def freeze(model, optimizer, pattern):
    import train
    if pattern in ("transfer", "prebias"):
        train.freeze_for_transfer(model, optimizer, transfer=pattern == "transfer", prebias=pattern == "prebias")
    elif pattern == "trunk":
        for k, p in model.named_parameters():
            p.requires_grad = int(k.split(".")[1]) >= 75
    return sum(p.numel() for p in model.parameters() if p.requires_grad), sum(1 for p in model.parameters() if p.requires_grad)


def make_step(pattern, bs, size, dev):
    """bench.py's bench_train step (hip backend, fused loss, one rank) on a model frozen to `pattern`"""
    import torch
    import train
    from bench import init_bench_weights
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.dist import GradientAllReducer
    from rotate_yolov3_amd.model.loss import compute_loss
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.utils.synthetic import synthetic_targets
    hyp = dict(HYP)
    torch.manual_seed(0)
    model = init_bench_weights(Darknet(make_cfg.darknet53(size, size), hyp), seed=0).to(dev).train()
    model.nc, model.arc, model.hyp = 1, "default", hyp
    model.enable_fused_loss(capacity=max(256, 8 * bs))
    opt = train.make_optimizer(model, hyp)
    counts = freeze(model, opt, pattern)
    dp = GradientAllReducer(model)          # after the freeze, as train.py does: the engine's kernels write the buckets directly
    x = torch.rand(bs, 3, size, size, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
    tg = synthetic_targets(bs, seed=1, device=dev)

    def step():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            pred = model(x)
        loss, items = compute_loss([p.float() for p in pred], tg.clone(), model, hyp)
        loss.backward()
        dp.finish()
        opt.step()
        dp.zero_grad()
        return items

    return model, step, counts


def engine_of(model):
    return [e for e in model._engines.values() if hasattr(e, "bplan")][0]


class CountingLib(object):
    """the library with every launch call counted (queries -- *_bytes, *_supported, *_rows -- are not launches)"""

    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        f = getattr(self.real, name)
        if not name.startswith("ryolo_") or name.endswith(("_bytes", "_supported", "_rows")):
            return f

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a)
        return call


def child(a):
    import torch
    from rotate_yolov3_amd import _lib
    dev = torch.device("cuda:0")         # (a fresh process: the peak counts from zero)
    model, step, (nelem, ntens) = make_step(a.child, a.bs, a.size, dev)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev)
    eng = engine_of(model)
    graphs = eng.g_fwd is not None and all(g is not None for g in eng.g_bwd or [None])
    # one more step with the backward launched eagerly through a counting proxy of the library
    real, launch = _lib.lib(), eng._backward_launch
    proxy = CountingLib(real)

    def counted(lo=0, hi=None):
        _lib.lib = lambda: proxy
        try:
            return launch(lo, hi)
        finally:
            _lib.lib = lambda: real
    eng._backward_launch, eng.force_eager = counted, True
    step()
    torch.cuda.synchronize(dev)
    entries = {}
    for kind, _, _, _ in eng.bplan:
        entries[kind] = entries.get(kind, 0) + 1
    print("FREEZE_CHILD " + json.dumps(dict(pattern=a.child, peak_bytes=peak, launches=sum(proxy.calls.values()), by_call=proxy.calls,
                                            entries=entries, trainable_tensors=ntens, trainable_elements=nelem, graphs=bool(graphs),
                                            direct_sink=bool(eng.direct), plan_buffers=len(eng._tplan.buffers))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5, help="steps before anything is measured: two eager, the capture, two replays")
    ap.add_argument("--child", default="", help="(internal) one pattern in this process: peak memory and backward launches")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.rounds < 5 or a.warmup < 4:
        ap.error("at least five rounds, and a warm-up past the graph capture (4 steps)")
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("freeze_step_bench: no GPU -- nothing is measured on the host")
    if a.child:
        return child(a)
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("freeze_step_bench: Darknet-53 %dx%d, bs %d, bench.py's training step (hip backend, fused loss, FusedSGD), one MI355X"
        % (a.size, a.size, a.bs))
    # ---- memory and launches: each pattern alone in a fresh process
    kids = {}
    for name in PATTERNS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--bs", str(a.bs), "--size", str(a.size),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("FREEZE_CHILD ")]
        if r.returncode != 0 or not got:
            raise SystemExit("child %s failed (exit %s):\n%s" % (name, r.returncode, (r.stdout + r.stderr)[-3000:]))
        kids[name] = json.loads(got[-1][len("FREEZE_CHILD "):])
    # ---- times: all four in this process, interleaved
    runs = [(name,) + make_step(name, a.bs, a.size, dev) for name in PATTERNS]
    for name, model, step, _ in runs:
        for _ in range(a.warmup):
            step()
        eng = engine_of(model)
        assert eng.g_fwd is not None and all(g is not None for g in eng.g_bwd), "%s: the step is not replayed from graphs" % name
    torch.cuda.synchronize(dev)
    times = dict((name, []) for name in PATTERNS)
    for r in range(a.rounds):
        for name, model, step, _ in (runs if r % 2 == 0 else runs[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.per_round):
                step()
            e1.record()
            torch.cuda.synchronize(dev)
            times[name].append(e0.elapsed_time(e1) / a.per_round)
    say("%d interleaved rounds of %d steps after %d warm-up steps (graphs captured), order reversed on odd rounds; ms per optimizer step "
        "between two device events" % (a.rounds, a.per_round, a.warmup))
    say("peak memory: torch.cuda.max_memory_allocated of a fresh process after %d steps; backward launches: C ABI launch calls of one "
        "eagerly launched backward" % a.warmup)
    say("%-9s %9s %9s %9s %7s %10s %9s %9s %8s   %s" % ("pattern", "median ms", "min", "max", "/ all", "peak GB", "launches", "entries",
                                                          "tensors", "rounds"))
    base = statistics.median(times["all"])
    for name in PATTERNS:
        t, k = times[name], kids[name]
        say("%-9s %9.3f %9.3f %9.3f %7.3f %10.2f %9d %9d %8d   %s"
            % (name, statistics.median(t), min(t), max(t), statistics.median(t) / base, k["peak_bytes"] / 1e9, k["launches"],
               sum(k["entries"].values()), k["trainable_tensors"], " ".join("%.2f" % v for v in t)))
    say()
    for name in PATTERNS:
        k = kids[name]
        say("%-9s %d trainable elements; backward entries %s; plan buffers %d; direct gradient sink %s; launch calls: %s"
            % (name, k["trainable_elements"], json.dumps(k["entries"], sort_keys=True), k["plan_buffers"], k["direct_sink"],
               ", ".join("%s %d" % (n.replace("ryolo_", ""), c) for n, c in sorted(k["by_call"].items()))))
    for name in PATTERNS[1:]:
        wins = sum(f < t for f, t in zip(times[name], times["all"]))
        say("%s faster than all in %d of %d rounds" % (name, wins, a.rounds))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
