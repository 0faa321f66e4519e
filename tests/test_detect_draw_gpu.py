"""GPU tier: the entry points of the drawing feature -- detect.py --save-img on the five procedural pictures of
tests/test_detect_images_gpu.py (its model, calibration and threshold, imported, not edited), utils.plots.plot_images and
train.py --plot-batch.  Every saved PNG is compared byte for byte with the oracle drawing (tests/draw_reference.py) of the original
picture, made from the rows of <stem>.txt of the same run and the class_colors / line_thickness / render_label outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.model.nhwc_batch import NHWC8Batch
from rotate_yolov3_amd.utils import plots
from tests import draw_reference as ref
from tests import test_detect_images_gpu as base
from tests.test_detect_images_gpu import folder, loaded, model, thr  # noqa: F401  (fixtures: the pictures, the calibrated model, the threshold)

import detect

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'), dtype=np.uint8)


def pictures_of(out):
    return {n: decode(os.path.join(out, n)) for n in sorted(os.listdir(out)) if n.endswith('.png')}


def oracle_picture(original, txt, thick=None):
    """the drawing of one picture from the text rows `x y w h a conf cls` of its result file"""
    rows = np.array([[float(v) for v in ln.split()] for ln in txt.splitlines()], dtype=np.float64).reshape(-1, 7)
    det = np.zeros((len(rows), 8))
    det[:, :6], det[:, 7] = rows[:, :6], rows[:, 6]
    quad, xy = ref.corners(det)
    assert ((np.abs(xy - np.rint(xy)) > 1e-4).all(1) | (det[:, 4] == 0)).all(), "a corner too close to an integer for the %g angle of the file"
    h, w = original.shape[:2]
    t = plots.line_thickness(h, w) if thick is None else thick
    table = plots.class_colors(plots.DEFAULT_CLASSES)
    colors = np.array([table[int(c) % len(table)] for c in det[:, 7]], dtype=np.uint8).reshape(-1, 3)
    labels = plots.pack_labels([plots.render_label(plots.label_text(None, c, s), t) for c, s in zip(det[:, 7], det[:, 5])], quad[:, :2])
    return ref.draw_image(original, quad, colors, t, labels)


@pytest.fixture(scope="module")
def runs(cuda_dev, model, thr, folder, tmp_path_factory):  # noqa: F811
    """detect.py on the folder: plain, with --save-img (batch 5 and 2), with --line-thickness 1 and 3; all with --icdar"""
    root = tmp_path_factory.mktemp("detect_draw")
    mp = pytest.MonkeyPatch()
    outs = {}
    try:
        for name, kw in (("plain", {}), ("img", dict(save_img=True)), ("img_bs2", dict(save_img=True, batch_size=2)),
                         ("thin", dict(save_img=True, line_thickness=1)), ("thick", dict(save_img=True, line_thickness=3))):
            outs[name] = str(root / name)
            detect.detect(base.make_opt(model, mp, cuda_dev, source=folder, output=outs[name], conf_thres=thr, icdar=True,
                                        data=str(root / "no.data"), **kw))
    finally:
        mp.undo()
    return outs


def test_save_img_writes_the_oracle_drawing_of_every_source(runs, folder):  # noqa: F811
    got = pictures_of(runs["img"])
    assert sorted(got) == sorted(base.NAMES)
    texts = base.files_of(runs["img"])
    originals = dict(zip(base.NAMES, base.make_images()))
    changed = 0
    for name in base.NAMES:
        txt = texts[os.path.splitext(name)[0] + '.txt']
        want = oracle_picture(originals[name], txt)
        assert got[name].shape == want.shape and np.array_equal(got[name], want), name
        if txt == '':
            assert np.array_equal(got[name], originals[name]), name          # no detection: saved unchanged
        changed += not np.array_equal(got[name], originals[name])
    assert any(t == '' for t in texts.values())
    assert changed >= 1                                   # the threshold fixture cannot make this vacuous
    assert all(np.array_equal(decode(os.path.join(folder, n)), originals[n]) for n in base.NAMES)      # the sources stay


def test_save_img_changes_no_other_file(runs):
    assert base.files_of(runs["img"]) == base.files_of(runs["plain"]) and len(base.files_of(runs["plain"])) == 5
    assert base.files_of(os.path.join(runs["img"], 'icdar')) == base.files_of(os.path.join(runs["plain"], 'icdar'))
    import zipfile                                        # (a zip carries time stamps: its members are compared)
    with zipfile.ZipFile(os.path.join(runs["img"], 'icdar_result.zip')) as a, zipfile.ZipFile(os.path.join(runs["plain"], 'icdar_result.zip')) as b:
        assert a.namelist() == b.namelist() and all(a.read(n) == b.read(n) for n in a.namelist())
    assert pictures_of(runs["plain"]) == {} and sorted(os.listdir(runs["plain"])) == sorted(set(os.listdir(runs["img"])) - set(base.NAMES))


def test_batch_size_two_gives_the_same_pictures(runs):
    a, b = pictures_of(runs["img"]), pictures_of(runs["img_bs2"])
    assert sorted(a) == sorted(b) == sorted(base.NAMES) and all(np.array_equal(a[n], b[n]) for n in a)


def test_line_thickness_overrides_the_formula_as_the_oracle_says(runs):
    """The five pictures are at most 200 pixels wide, where line_thickness() is round(0.002 (h + w) / 2) + 1 = 1 already: --line-thickness 1
    must give the default's pictures there, and it is --line-thickness 3 that changes them.  Both equal the oracle at their thickness."""
    assert all(plots.line_thickness(h, w) == 1 for h, w in base.SIZES)
    a, thin, thick = pictures_of(runs["img"]), pictures_of(runs["thin"]), pictures_of(runs["thick"])
    originals = dict(zip(base.NAMES, base.make_images()))
    assert all(np.array_equal(a[n], thin[n]) for n in a)
    assert any(not np.array_equal(a[n], thick[n]) for n in a)
    for t, got, out in ((1, thin, runs["thin"]), (3, thick, runs["thick"])):
        texts = base.files_of(out)
        assert texts == base.files_of(runs["plain"])
        for name in base.NAMES:
            assert np.array_equal(got[name], oracle_picture(originals[name], texts[os.path.splitext(name)[0] + '.txt'], thick=t)), (t, name)


def test_class_names_come_from_the_data_file(cuda_dev, model, thr, folder, runs, tmp_path, monkeypatch, capsys):  # noqa: F811
    (tmp_path / "c.names").write_text("vessel\n")
    (tmp_path / "c.data").write_text("classes=1\nnames=%s\n" % (tmp_path / "c.names"))
    name = [n for n in base.NAMES if base.files_of(runs["plain"])[os.path.splitext(n)[0] + '.txt'] != ''][0]      # a picture with detections
    source = os.path.join(folder, name)
    for data, out in ((str(tmp_path / "c.data"), "named"), (str(tmp_path / "missing.data"), "unnamed")):
        detect.detect(base.make_opt(model, monkeypatch, cuda_dev, source=source, output=str(tmp_path / out), conf_thres=thr, save_img=True,
                                    data=data))
        printed = capsys.readouterr().out
        assert ('NOTE: --data' in printed) == (out == "unnamed")
    a, b = decode(str(tmp_path / "named" / name)), decode(str(tmp_path / "unnamed" / name))
    assert not np.array_equal(a, b)                       # 'vessel 0.xx' is not '0 0.xx'


def test_npy_source_with_save_img_prints_the_note_and_writes_no_image(cuda_dev, model, thr, tmp_path, monkeypatch, capsys):  # noqa: F811
    x = torch.rand(2, 3, base.S, base.S, generator=torch.Generator().manual_seed(3))
    np.save(str(tmp_path / 'x.npy'), x.numpy())
    out = str(tmp_path / 'npy')
    detect.detect(base.make_opt(model, monkeypatch, cuda_dev, source=str(tmp_path / 'x.npy'), output=out, conf_thres=thr, save_img=True,
                                line_thickness=2))
    assert 'NOTE: --save-img, --line-thickness: only for a --source of image files' in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ['img_0.txt', 'img_1.txt']


# ---- plot_images, train.py --plot-batch

def known_batch(cuda_dev):
    x = torch.rand(5, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    data = torch.zeros(5, 64, 64, 8, dtype=torch.bfloat16)
    data[..., :3] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    targets = torch.tensor([[0, 0, 0.5, 0.5, 0.6, 0.2, 0.4], [0, 0, 0.3, 0.7, 0.2, 0.5, -1.2], [2, 0, 0.5, 0.5, 0.9, 0.9, 0.0],
                            [4, 0, 0.8, 0.2, 0.5, 0.1, 1.5], [1, 0, 0.1, 0.1, 0.4, 0.3, 0.7], [4, 0, 0.5, 0.5, 0.3, 0.3, -0.3]])
    return NHWC8Batch(data.to(cuda_dev)), targets.to(cuda_dev), data


def test_plot_images_is_the_torch_mosaic_plus_the_oracle_drawing(cuda_dev, tmp_path):
    batch, targets, data = known_batch(cuda_dev)
    before = batch.data.clone()
    got = plots.plot_images(batch, targets, str(tmp_path / 'b.png'), seed=4)
    assert torch.equal(batch.data, before)
    mosaic = np.zeros((192, 192, 3), dtype=np.uint8)
    cells = (data[..., :3].float() * 255.0).to(torch.uint8).numpy()           # truncated, on the CPU
    for i in range(5):
        mosaic[(i // 3) * 64:(i // 3 + 1) * 64, (i % 3) * 64:(i % 3 + 1) * 64] = cells[i]
    det = plots.mosaic_rows(targets.cpu().numpy(), 5, 3, 64, 64)
    quad, xy = ref.corners(det)
    assert len(det) == 6 and ((np.abs(xy - np.rint(xy)) > 1e-6).all(1) | (det[:, 4] == 0)).all()
    colors = np.random.default_rng(4).integers(0, 256, (6, 3), dtype=np.uint8)
    want = ref.draw_image(mosaic, quad, colors, 2)
    saved = decode(str(tmp_path / 'b.png'))
    assert saved.shape == (192, 192, 3) and np.array_equal(saved, want) and np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, mosaic)
    assert not saved[128:, 64:].any() and not saved[64:128, 128:].any()     # cells 5..8 are zero
    plots.plot_images(batch, targets, str(tmp_path / 'b.jpg'), seed=4)
    assert decode(str(tmp_path / 'b.jpg')).shape == (192, 192, 3)


@pytest.mark.parametrize("flag", [["--plot-batch"], []], ids=["with", "without"])
def test_train_py_plot_batch_leaves_the_mosaic_and_only_with_the_flag(cuda_dev, tmp_path, flag):
    """train.py as tests/test_train_entry.py runs it (its hyp file, 64 pixels, synthetic images), on the GPU with the tiny cfg the other GPU
    runs of train.py use: the 8- and 16-channel cfg of the CPU tier is not a HIP TrainEngine shape"""
    from tests.test_train_engine_gpu import MINI_CFG
    (tmp_path / "m.cfg").write_text(MINI_CFG)
    (tmp_path / "hyp.py").write_text("giou: 0.1\ncls: 27.76\ncls_pw: 1.446\nobj: 20.35\nobj_pw: 3.941\niou_t: 0.3\nang_t: 3.1415926/12\n"
                                     "reg: 1.0\nfl_gamma: 0.5\ncontext_factor: 1.0\nlr0: 0.0001\nmultiplier:10\nwarm_epoch:1\nmomentum: 0.97\n"
                                     "weight_decay: 0.0004569\nepochs: 1\nbatch_size: 2\nsave_interval: 300\ntest_interval: 5\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--cfg", str(tmp_path / "m.cfg"), "--hyp", str(tmp_path / "hyp.py"),
                        "--img-size", "64", "--synthetic", "2", "--notest", "--device", "0", "--wdir", str(tmp_path / "w")] + flag,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.isfile(str(tmp_path / "w" / "last.pt"))
    assert os.path.isfile(str(tmp_path / "train_batch0.jpg")) == bool(flag)
    if flag:
        assert decode(str(tmp_path / "train_batch0.jpg")).shape == (128, 128, 3)      # two images: a 2 x 2 mosaic of 64 x 64 cells
        assert "--plot-batch: wrote train_batch0.jpg" in r.stdout
