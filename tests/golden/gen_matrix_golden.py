"""Generate the golden vectors of the matrix model FROM THE REFERENCE's own Python (its Darknet with `weight_from` / `d-convolutional`
blocks, model/models.py:68-77, :254-265), imported with the stub modules of gen_model_golden.py.  Nothing of the reference is written
into the repo: only inputs and expected outputs (.npz).

    python tests/golden/gen_matrix_golden.py        (needs /root/reference)

Fixture:
  forward_matrix_96.npz  the reference Darknet on the make_cfg.darknet53_matrix(96, 96, na_per_head=8) cfg text (maps 12^2 / 6^2 / 3^2, 2^2
                         for the stride-64 head; 16 heads of width 56; dilations (1,2) (2,1) (1,4) (4,1) (1,8) (8,1)), fill_procedural
                         weights with the shared source convs refilled by tests/matrix_reference.fill_matrix, on rand(1,3,96,96) seed 0: x, io (all 16 heads), p0..p3
                         (the FPN and stride-64 heads; the p of the twelve matrix heads are the rows of io before the decode and would
                         double the file), mean |p| of every head (p_mean), the ordered state_dict keys
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from tests.golden.gen_model_golden import REF, install_stubs  # noqa: E402
from tests.matrix_reference import SHARED_AMP, fill_matrix  # noqa: E402
from tests.procedural import fill_procedural  # noqa: E402

MODEL_BAR = (0.015, 0.0025)      # max rel / mean rel of the engine-vs-emulation tests (tests/test_model_gpu._cmp)


def rel(a, b):
    """(max rel, mean rel) in the terms of tests/test_model_gpu._cmp"""
    scale = b.abs().mean().item() + 1e-6
    err = (a - b).abs()
    return (err / (b.abs() + scale)).max().item(), err.mean().item() / scale


def main():
    assert os.path.isdir(REF)
    install_stubs()
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    from model import models as rmodels
    sys.path.insert(0, ROOT)
    import rotate_yolov3_amd  # noqa: F401
    from rotate_yolov3_amd.cfg import make_cfg

    cfg_path = os.path.join(tempfile.mkdtemp(), "d53matrix.cfg")
    open(cfg_path, "w").write(make_cfg.darknet53_matrix(96, 96, na_per_head=8))
    model = rmodels.Darknet(cfg_path, {"context_factor": 1.0}).eval()
    fill_matrix(fill_procedural(model))
    x = torch.rand(1, 3, 96, 96, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        io, p = model(x)
    assert len(p) == 16 and bool(torch.isfinite(io).all())
    means = [float(q.abs().mean()) for q in p]
    for k, q in enumerate(p):
        print("head %2d  %s  mean |p| %.4g  max |p| %.4g" % (k, tuple(q.shape), means[k], float(q.abs().max())))
    for k in range(4, 16):
        assert means[k] >= 0.1, "matrix head %d has mean |p| %.3g with SHARED_AMP %s -- change it (tests/matrix_reference.py)" % (k, means[k], SHARED_AMP)
    # heads 10 and 11: the (1,2) and (2,1) branches of the 12^2 level -- a kernel that swapped dh and dw must not pass as one of them
    d_max, d_mean = rel(p[10], p[11])
    print("12^2 level, (1,2) head vs (2,1) head: max rel %.4g  mean rel %.4g" % (d_max, d_mean))
    assert d_max > 10 * MODEL_BAR[0] and d_mean > 10 * MODEL_BAR[1], (d_max, d_mean)
    path = os.path.join(OUT, "forward_matrix_96.npz")
    np.savez_compressed(path, x=x.numpy(), io=io.numpy(), p_mean=np.array(means), keys=np.array(list(model.state_dict().keys())),
                        **{"p%d" % k: p[k].numpy() for k in range(4)})
    os.chdir(cwd)
    print("io", tuple(io.shape), "file %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
