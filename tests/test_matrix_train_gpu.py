"""GPU tier of training a matrix cfg through the ATen chain with its dilated shared convs on the HIP kernels
(Darknet.shared_conv_backend = 'hip'): parity with the CPU emulation of SharedDilatedConv, bit reproducibility, the unchanged default
and the per-model cache of packed weight images.  The model is the mini cfg of tests/matrix_train_reference.py at 64^2 input, bs 2; the
scalar is sum_k <p_k, r_k> with fixed random r_k, so the loss code is not under test.

Parity bar: the project's per-block dW bar, cosine >= 0.9999 and max|err| <= 2e-3 max|g| + 1e-3, against the emulation
that accumulates in fp32.  Fair: on the CPU the emulation with fp64 accumulation differs from the one with fp32 accumulation by 6.4e-3
(stem) and 4.1e-3 (layer A) against half bars of 0.22 and 0.18 (tests/test_matrix_train_cpu.py asserts it)."""
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
import oracle
from rotate_yolov3_amd.model import hip_train_ops as T
from tests import matrix_train_reference as R

pytestmark = pytest.mark.gpu
torch.set_num_threads(oracle.host_cores(16))


@pytest.fixture()
def deterministic_aten():
    """the ATen layers around the HIP ones must not add run-to-run noise of their own to the bit comparisons"""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _gpu_model(dev, backend):
    m = R.make_model().to(dev)
    m.backend = "torch"
    m.shared_conv_backend = backend
    return m


def _step(m, x, rs):
    return R.grads(m, m(x), rs)


@pytest.fixture(scope="module")
def emulation():
    """the CPU emulation's gradients, once"""
    m = R.make_model()
    x = R.make_input()
    rs = R.fixed_r(m(x))
    return x, rs, R.grads(m, R.chain(m, x, R.emulated(torch.float32)), rs)


def test_hip_shared_convs_match_the_emulation(cuda_dev, emulation):
    x, rs, want = emulation
    m = _gpu_model(cuda_dev, "hip")
    got = _step(m, x.to(cuda_dev), rs)
    torch.cuda.synchronize()
    for k, name in ((R.A, "A"), (R.STEM, "stem")):        # A: its own gradient + the two sharers'; the stem's passes through both data gradients
        err = float((got[k].cpu() - want[k]).abs().max())
        cos = R.cosine(got[k], want[k])
        print("%s: max err %.4g, bar %.4g, max |g| %.4g, cosine %.8f" % (name, err, R.dw_bar(want[k]), float(want[k].abs().max()), cos))
        assert cos >= 0.9999 and err <= R.dw_bar(want[k]), (name, err, cos)


def test_hip_step_is_bit_reproducible(cuda_dev, emulation, deterministic_aten):
    x, rs, _ = emulation
    m = _gpu_model(cuda_dev, "hip")
    xd = x.to(cuda_dev)
    a = _step(m, xd, rs)
    b = _step(m, xd, rs)
    torch.cuda.synchronize()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_default_backend_is_the_plain_aten_chain(cuda_dev, emulation, deterministic_aten):
    """shared_conv_backend = 'torch' (the default): the gradients of Darknet's forward equal those of the F.conv2d restatement bit for bit"""
    x, rs, _ = emulation
    m = R.make_model().to(cuda_dev)
    m.backend = "torch"
    assert m.shared_conv_backend == "torch"
    xd = x.to(cuda_dev)
    got = _step(m, xd, rs)
    want = R.grads(m, R.chain(m, xd), rs)
    torch.cuda.synchronize()
    assert all(torch.equal(got[k], want[k]) for k in got)
    assert "shared_conv_packs" not in m.__dict__


def test_unsupported_layer_raises_with_its_index(cuda_dev):
    """no silent fallback: a d-convolutional layer the kernels do not serve (32 channels) is an error that names the layer"""
    cfg = R.MINI_CFG.replace("filters=64", "filters=32")
    torch.manual_seed(0)
    from rotate_yolov3_amd.model.models import Darknet
    m = Darknet(cfg, {"context_factor": 1.0}).train().to(cuda_dev)
    m.backend, m.shared_conv_backend = "torch", "hip"
    with pytest.raises(RuntimeError, match="layer 5 "):
        m(R.make_input().to(cuda_dev))
    m.shared_conv_backend = "torch"
    assert len(m(R.make_input().to(cuda_dev))) == 2


def test_source_weight_is_packed_once_per_direction_per_step(cuda_dev, emulation, monkeypatch):
    x, rs, _ = emulation
    counts = {"fwd": 0, "dgrad": 0}
    real_f, real_d = T.pack_weights, T.pack_weights_dgrad

    def pack_f(*a, **k):
        counts["fwd"] += 1
        return real_f(*a, **k)

    def pack_d(*a, **k):
        counts["dgrad"] += 1
        return real_d(*a, **k)

    monkeypatch.setattr(T, "pack_weights", pack_f)
    monkeypatch.setattr(T, "pack_weights_dgrad", pack_d)
    m = _gpu_model(cuda_dev, "hip")
    xd = x.to(cuda_dev)
    _step(m, xd, rs)
    assert counts == {"fwd": 1, "dgrad": 1}, counts            # two sharers, one source: packed once per direction
    assert isinstance(m.shared_conv_packs, T.SharedConvPacks)  # the cache lives on the model
    _step(m, xd, rs)
    assert counts == {"fwd": 1, "dgrad": 1}, counts            # the weight did not change
    with torch.no_grad():
        m.module_list[R.A].Conv2d.weight.mul_(1.01)            # an optimizer step: in place, the version moves
    _step(m, xd, rs)
    assert counts == {"fwd": 2, "dgrad": 2}, counts
    other = _gpu_model(cuda_dev, "hip")                        # another model has its own cache
    _step(other, xd, rs)
    assert counts == {"fwd": 3, "dgrad": 3}, counts
    torch.cuda.synchronize()
