"""Generate the golden vectors of the squeeze-and-excitation model FROM THE REFERENCE's own Python (its Darknet / SELayer,
model/models.py:16-31, :89-91), imported with the stub modules of gen_model_golden.py.  Nothing of the reference is written
into the repo: only inputs and expected outputs (.npz).

    python tests/golden/gen_se_golden.py        (needs /root/reference)

Fixture:
  forward_d53se_64.npz  the reference Darknet on the make_cfg.darknet53_se(64, 64) cfg text, fill_procedural weights with the se
                        weights of tests/se_reference.fill_se, on rand(1,3,64,64) seed 0: x, io, p0..p2, the 20 gate vectors
                        (gate_<layer>), the ordered state_dict keys
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
from tests.procedural import fill_procedural  # noqa: E402
from tests.se_reference import SE_AMP, fill_se  # noqa: E402


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

    cfg_path = os.path.join(tempfile.mkdtemp(), "d53se.cfg")
    open(cfg_path, "w").write(make_cfg.darknet53_se(64, 64))
    model = rmodels.Darknet(cfg_path, {"context_factor": 1.0}).eval()
    fill_se(fill_procedural(model))
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    gates = {}

    def hook(i):
        def fn(m, inp, out):
            gates[i] = out.reshape(-1).clone()        # fc = Linear, ReLU, Linear, Sigmoid: its output is the gate vector
        return fn
    for i, (d, m) in enumerate(zip(model.module_defs, model.module_list)):
        if d["type"] == "se":
            m.fc.register_forward_hook(hook(i))
    with torch.no_grad():
        io, p = model(x)
    assert len(gates) == 20
    for i, g in sorted(gates.items()):
        print("se %3d  C %4d  gate min %.3f max %.3f" % (i, g.numel(), float(g.min()), float(g.max())))
        assert float(g.min()) < 0.35 and float(g.max()) > 0.65, \
            "se %d: gates stay in [%.3f, %.3f] with SE_AMP %g -- raise it (tests/se_reference.py)" % (i, float(g.min()), float(g.max()), SE_AMP)
    path = os.path.join(OUT, "forward_d53se_64.npz")
    np.savez_compressed(path, x=x.numpy(), io=io.numpy(), p0=p[0].numpy(), p1=p[1].numpy(), p2=p[2].numpy(),
                        keys=np.array(list(model.state_dict().keys())), **{"gate_%d" % i: g.numpy() for i, g in gates.items()})
    os.chdir(cwd)
    print("io", tuple(io.shape), "file %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
