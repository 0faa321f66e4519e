"""GPU tier: detect.py --nms-style on image files at two scales, as a child process per style -- a random-weight two-class tiny cfg, two
generated pictures.  Both styles keep the same rows (MERGE only moves boxes), and the MERGE files are the rows of
utils.detect_images.detect_images(..., nms_style='MERGE') called in this process on the same weights."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.utils import datasets as ds
from rotate_yolov3_amd.utils.detect_images import detect_images
from tests.test_cabi import ROOT

pytestmark = pytest.mark.gpu

SCALES = (64, 96)
NMS = 0.3
SIZES = [(90, 120), (96, 64)]          # (h, w)


def row_text(rows):
    return ''.join(('%g ' * 7 + '\n') % (*box, conf, cls) for *box, conf, _, cls in rows)


def test_detect_py_nms_style_children_and_in_process(cuda_dev, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(17)
    folder = tmp_path / 'img'
    folder.mkdir()
    for name, (h, w) in zip(('a.png', 'b.png'), SIZES):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        a = np.stack([127 + 120 * np.sin(x / 7 + y / 13), 127 + 120 * np.cos(x / 5), rng.integers(0, 256, (h, w))], 2)
        Image.fromarray(np.clip(np.rint(a), 0, 255).astype(np.uint8)).save(str(folder / name))
    cfg = tmp_path / 'tiny2.cfg'
    cfg.write_text(make_cfg.tiny(96, 96, classes=2))          # two classes: 36 x 8 head channels, a shape of the HIP path
    torch.manual_seed(23)
    model = Darknet(str(cfg), {'context_factor': 1.0})
    weights = tmp_path / 'w.pt'
    torch.save({'model': model.state_dict()}, str(weights))
    model.to(cuda_dev).eval()

    (paths, cache, shapes), = list(ds.LoadImages(str(folder), 96, 2, cuda_dev))
    # a threshold that about a fifth of the rows pass at the smaller scale: many overlapping candidates per image, at both scales
    with torch.no_grad():
        io = model(ds.letterbox_batch(cache, shapes, SCALES[0], 2))[0].float()
    score = (io[..., 5] * io[..., 6:].max(2)[0]).flatten()
    conf = float(score.kthvalue(int(score.numel() * 0.8)).values)
    want, _, _ = detect_images(model, cache, 2, shapes, SCALES, conf, NMS, slots=2, nms_style='MERGE')
    plain, _, _ = detect_images(model, cache, 2, shapes, SCALES, conf, NMS, slots=2)
    assert all(r is not None for r in want)

    files = {}
    for style in ('OR', 'MERGE'):
        out = tmp_path / style
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'detect.py'), '--cfg', str(cfg), '--hyp', '', '--weights', str(weights),
                            '--source', str(folder), '--output', str(out), '--img-size', '96', '--scales', '64,96', '--conf-thres',
                            repr(conf), '--nms-thres', repr(NMS), '--batch-size', '2', '--device', '0', '--nms-style', style],
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        assert 'use scale: [64, 96]' in r.stdout
        files[style] = {n: open(str(out / n)).read() for n in sorted(os.listdir(str(out))) if n.endswith('.txt')}
    assert sorted(files['OR']) == sorted(files['MERGE']) == ['a.txt', 'b.txt']
    moved = 0
    for p, rows, prow in zip(paths, want, plain):
        stem = os.path.splitext(os.path.basename(p))[0] + '.txt'
        assert files['MERGE'][stem] == row_text(rows.cpu().tolist()), stem
        assert files['OR'][stem] == row_text(prow.cpu().tolist()), stem
        assert len(files['OR'][stem].splitlines()) == len(files['MERGE'][stem].splitlines()) == len(rows) > 0
        assert torch.equal(rows[:, 5:], prow[:, 5:])
        moved += int((rows[:, :5] != prow[:, :5]).any(1).sum())
    print("rows per image %s, rows whose box MERGE moved: %d" % ([len(r) for r in want], moved))
