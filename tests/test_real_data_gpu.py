"""GPU tier: the real-data loader end to end (rotate-yolov3_amd/utils/datasets.py over csrc/augment.hip).  Six PNGs of three sizes, each
black but for a bright 5 x 5 blob at the centre of its one box, label files and a list file, all written to tmp_path.  The blob
ties the two halves together: the picture is warped on the device, the label on the host, and the blob must land where the label says."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd.model import hip_ops as ops  # noqa: E402
from rotate_yolov3_amd.model.nhwc_batch import NHWC8Batch  # noqa: E402
from rotate_yolov3_amd.utils import datasets as ds  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
SIZES = [(64, 64), (48, 80), (100, 60), (64, 64), (48, 80), (100, 60)]      # (h, w); the last two are reduced to a long side of 64
# geometry only: a blob has to stay a blob (the photometric stages have their own tests)
HYP = dict(degrees=10.0, translate=0.1, scale=0.15, shear=0.0, noise=0.0, gamma=0.0, blur=0.0, hsv_s=0.0, hsv_v=0.0, grayscale=1.0)
HYP_FILE = ("giou: 0.1\ncls: 27.76\ncls_pw: 1.0\nobj: 20.35\nobj_pw: 1.0\niou_t: 0.5\nang_t: 3.1415926/12\nreg: 1.0\nfl_gamma: 0.5\n"
            "context_factor: 1.0\nlr0: 0.0001\nmultiplier:10\nwarm_epoch:1\nmomentum: 0.97\nweight_decay: 0.0004569\nepochs: 1\n"
            "batch_size: 3\nsave_interval: 300\ntest_interval: 5\ndegrees: 10\ntranslate: 0.1\nscale: 0.15\nshear: 0\nnoise: 0.02\n"
            "gamma: 0.2\nblur: 1.0\nhsv_s: 0.3\nhsv_v: 0.3\ngrayscale: 0.5\n")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("hrsc")
    (root / "images").mkdir()
    (root / "labels").mkdir()
    rng = np.random.default_rng(8)
    paths, centres = [], []
    for k, (h, w) in enumerate(SIZES):
        cx, cy = int(rng.integers(w // 3, 2 * w // 3)), int(rng.integers(h // 3, 2 * h // 3))
        a = np.zeros((h, w, 3), dtype=np.uint8)
        a[cy - 2:cy + 3, cx - 2:cx + 3] = 255
        p = root / "images" / ("im%d.png" % k)
        Image.fromarray(a).save(str(p))
        # the blob covers pixels cx-2 .. cx+2: its centre is (cx + 0.5, cy + 0.5) in the labels' continuous coordinates
        (root / "labels" / ("im%d.txt" % k)).write_text("0 %.6f %.6f %.6f %.6f %.6f\n" % ((cx + 0.5) / w, (cy + 0.5) / h, 0.3, 0.2, 0.1 * k - 0.2))
        paths.append(str(p))
        centres.append((cx, cy))
    lst = root / "train.txt"
    lst.write_text("\n".join(paths + [str(root / "images" / "notes.md")]) + "\n")
    data = root / "hrsc.data"
    data.write_text("classes=1\ntrain=%s\nvalid=%s\nnames=none\n" % (lst, lst))
    hyp = root / "hyp.py"
    hyp.write_text(HYP_FILE)
    return dict(root=root, list=str(lst), data=str(data), hyp=str(hyp), paths=paths)


def _loader(dataset, dev, **kw):
    args = dict(img_size=S, batch_size=4, augment=True, hyp=HYP, seed=3, device=dev)
    args.update(kw)
    return ds.LoadImagesAndLabels(dataset["list"], **args)


def _centroid(img):
    """of what is brighter than the grey border (128 / 255) in one [3, H, W] image, in continuous coordinates (pixel i covers [i, i + 1))"""
    m = (img.mean(0).double() - 0.55).clamp(min=0)
    ys, xs = torch.meshgrid(torch.arange(m.shape[0], dtype=torch.float64), torch.arange(m.shape[1], dtype=torch.float64), indexing="ij")
    return float((m * xs).sum() / m.sum()) + 0.5, float((m * ys).sum() / m.sum()) + 0.5, float(m.sum())


def test_blobs_land_where_the_labels_say(cuda_dev, dataset):
    loader = _loader(dataset, cuda_dev)
    assert len(loader) == 2 and loader.cache.n == 6 and loader.cache.hw[4] == (38, 64) and loader.cache.shapes[4] == (48, 80)
    seen, warped = 0, 0
    for epoch in range(3):
        loader.set_epoch(epoch)
        for batch, targets, paths, shapes in loader:
            assert isinstance(batch, NHWC8Batch) and tuple(batch.shape)[1:] == (3, S, S) and len(paths) == len(batch) == len(shapes)
            assert targets.is_cuda and targets.shape[1] == 7 and targets.dtype == torch.float32
            imgs = batch.float().cpu()
            t = targets.cpu()
            for n in range(len(batch)):
                i = dataset["paths"].index(paths[n])
                assert shapes[n] == SIZES[i]
                warped += loader.draw(i).affine is not None
                rows = t[t[:, 0] == n]
                if len(rows) == 0:            # the box left the picture (random_affine's filter): nothing to compare
                    continue
                gx, gy, mass = _centroid(imgs[n])
                assert mass > 0.5          # of 25 * 0.45 for a whole blob at full size, about a third of that after the BOX reduction
                lx, ly = float(rows[0, 2]) * S, float(rows[0, 3]) * S
                assert abs(gx - lx) < 1.5 and abs(gy - ly) < 1.5, (epoch, paths[n], (gx, gy), (lx, ly), loader.draw(i))
                seen += 1
    assert seen >= 12 and warped >= 4, (seen, warped)


def test_same_seed_same_batches_and_shards_partition_the_epoch(cuda_dev, dataset):
    a, b = _loader(dataset, cuda_dev), _loader(dataset, cuda_dev)
    a.set_epoch(1)
    b.set_epoch(1)
    whole = list(a)
    for (xa, ta, pa, sa), (xb, tb, pb, sb) in zip(whole, list(b)):
        assert torch.equal(xa.data.view(torch.int16), xb.data.view(torch.int16)) and torch.equal(ta, tb) and pa == pb and sa == sb
    other = _loader(dataset, cuda_dev, seed=4)
    other.set_epoch(1)
    assert [p for _, _, p, _ in other] != [p for _, _, p, _ in whole] or not torch.equal(next(iter(other))[1], whole[0][1])
    # world = 2: the two ranks serve disjoint halves of the world = 1 epoch, image for image the same picture and label
    single = {}
    one = _loader(dataset, cuda_dev, batch_size=1)
    one.set_epoch(1)
    for x, t, p, _ in one:
        single[p[0]] = (x.data.view(torch.int16).clone(), t.clone())
    served = []
    for rank in (0, 1):
        shard = _loader(dataset, cuda_dev, batch_size=1, rank=rank, world=2)
        shard.set_epoch(1)
        assert len(shard) == 3
        for x, t, p, _ in shard:
            served.append(p[0])
            assert torch.equal(x.data.view(torch.int16), single[p[0]][0]) and torch.equal(t, single[p[0]][1])
    assert sorted(served) == sorted(single) == sorted(dataset["paths"])
    assert served[:3] == [ps[0] for _, _, ps, _ in one][0::2]          # rank 0 serves every second image of the epoch's order


def test_without_augmentation_the_loader_is_the_identity_letterbox(cuda_dev, dataset):
    loader = _loader(dataset, cuda_dev, augment=False, batch_size=6)
    (batch, targets, paths, shapes), = list(loader)
    assert list(paths) == dataset["paths"]
    for n, (h, w) in enumerate(SIZES):
        with Image.open(paths[n]) as im:
            if max(h, w) > S:
                im = im.resize(ds.letterbox_matrix(h, w, S).new_unpad, Image.BOX)
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        lb = ds.letterbox_matrix(a.shape[0], a.shape[1], S)
        want = np.full((S, S, 3), 128, dtype=np.uint8)
        want[lb.top:lb.top + a.shape[0], lb.left:lb.left + a.shape[1]] = a
        x32 = torch.from_numpy(want.astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None].contiguous().to(cuda_dev)
        assert torch.equal(ops.nchw_f32_to_nhwc_bf16(x32).view(torch.int16), batch.data[n:n + 1].view(torch.int16)), paths[n]
    # and the labels are the reference's letterbox arithmetic: ratio * w * x + dw, normalised
    t = targets.cpu().numpy()
    assert t.shape == (6, 7) and list(t[:, 0]) == list(range(6))
    h, w = loader.cache.hw[1]
    lab = ds.read_labels(ds.label_path_of(paths[1]))
    lb = ds.letterbox_matrix(h, w, S)
    assert abs(t[1, 2] * S - (lb.ratio * w * lab[0, 1] + lb.dw)) < 1e-3 and abs(t[1, 6] - lab[0, 5]) < 1e-6
    with pytest.raises(NotImplementedError):
        ds.LoadImagesAndLabels(dataset["list"], S, 2, rect=True, device=cuda_dev)
    with pytest.raises(NotImplementedError):
        ds.LoadImagesAndLabels(dataset["list"], S, 2, image_weights=True, device=cuda_dev)
    with pytest.raises(RuntimeError, match="cache_limit_bytes"):
        ds.LoadImagesAndLabels(dataset["list"], S, 2, device=cuda_dev, cache_limit_bytes=20000)


def _cfg(tmp_path):
    from tests.test_train_engine_gpu import MINI_CFG
    cfg = tmp_path / "mini.cfg"
    cfg.write_text(MINI_CFG)
    return str(cfg)


def test_train_py_real_data_runs_two_steps_with_a_finite_loss(cuda_dev, dataset, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--cfg", _cfg(tmp_path), "--hyp", dataset["hyp"], "--data", dataset["data"],
                        "--img-size", str(S), "--real-data", "--notest", "--device", "0", "--wdir", str(tmp_path / "w")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "non-finite" not in r.stdout
    rows = (tmp_path / "results.txt").read_text().strip().split("\n")
    assert len(rows) == 1
    losses = [float(v) for v in rows[0].split()[2:6]]
    assert all(np.isfinite(losses)) and losses[3] > 0, rows[0]
    assert os.path.isfile(str(tmp_path / "w" / "last.pt"))


def test_test_py_real_data_runs_an_evaluation_to_the_end(cuda_dev, dataset, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--cfg", _cfg(tmp_path), "--hyp", dataset["hyp"], "--data", dataset["data"],
                        "--img-size", str(S), "--batch-size", "4", "--real-data", "--device", "0", "--conf-thres", "0.5", "--weights", ""],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("all")]
    assert line and line[0].split()[1] == "6", r.stdout[-2000:]      # six images seen
