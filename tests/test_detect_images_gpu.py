"""GPU tier: detect.py on image files -- LoadImages, ryolo_letterbox_area, Darknet.detect, ryolo_det_rescale / ryolo_det_quads, the result
files -- and utils.detect_images.detect_images at several scales against the reference's multi_detect flow restated on the CPU.

Five procedural PNGs go to a temporary folder: two with a long side above the network size (96), one smaller, two with a side equal to
it.  The model is the procedural-weight Darknet-53 with its BatchNorm statistics taken from the five pictures and its heads scaled down
(calibrate: the plain procedural network's scores do not depend on the picture).  The confidence threshold is chosen on the CPU from a
first forward at the three sizes (choose_threshold): the lowest score level that leaves one image without any detection and another one
without a detection at one scale but with detections at another."""
import argparse
import os
import zipfile

import numpy as np
import pytest
import torch

import rotate_yolov3_amd  # noqa: F401
from oracle import darknet_oracle as do
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model.models import Darknet
from rotate_yolov3_amd.utils import datasets as ds
from rotate_yolov3_amd.utils.detect_images import detect_images, rescale_geometry
from rotate_yolov3_amd.utils.icdar import icdar_name
from tests import detect_reference as dref
from tests.procedural import fill_procedural

import detect

pytestmark = pytest.mark.gpu

S = 96
SCALES = (64, 96, 128)
NMS = 0.3
HEAD_GAIN = 0.05
SIZES = [(150, 200), (130, 97), (60, 80), (96, 96), (96, 64)]          # (h, w)
NAMES = ['e_wide.png', 'a_tall.png', 'c_small.png', 'b_square.png', 'd_half.png']


def make_images():
    """five RGB uint8 pictures of SIZES, each a different procedure: waves, a checkerboard, a ramp, bright boxes on black, noise"""
    rng = np.random.default_rng(31)
    out = []
    for k, (h, w) in enumerate(SIZES):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        if k == 0:
            a = np.stack([127 + 120 * np.sin(x / 7 + y / 13), 127 + 120 * np.cos(x / 5), 127 + 120 * np.sin(y / 3)], 2)
        elif k == 1:
            a = np.repeat((((x // 8) + (y // 8)) % 2 * 255)[..., None], 3, 2)
        elif k == 2:
            a = np.stack([x * 255 / w, y * 255 / h, 255 - x * 255 / w], 2)
        elif k == 3:
            a = np.zeros((h, w, 3))
            a[20:40, 10:70] = (250, 240, 20)
            a[60:75, 30:90] = (20, 200, 250)
        else:
            a = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
        out.append(np.clip(np.rint(a), 0, 255).astype(np.uint8))
    return out


def calibrate(model, images):
    """The procedural weights alone give a network whose output hardly depends on its input (its scores differ by 1e-5 between two
    pictures): no threshold could tell images apart.  One training-mode forward of the five pictures at each of SCALES on the CPU, with
    every BatchNorm averaging cumulatively, makes the running statistics those of the pictures, so every layer passes a signal on."""
    from tests import letterbox_area_reference as lref
    shapes = [a.shape[:2] for a in images]
    xs = [lref.letterbox_area(images, list(range(len(images))), ds.place_rows(shapes, size), size, size) for size in SCALES]
    xs = [torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2).contiguous() for x in xs]
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    saved = [m.momentum for m in bns]
    for m in bns:
        m.reset_running_stats()
        m.momentum = None
    model.train()
    with torch.no_grad():
        for x in xs:
            model(x)
    model.eval()
    for m, mom in zip(bns, saved):
        m.momentum = mom
    # with unit-variance features the three head convolutions (no BatchNorm behind them) put out tens: exp() of that is a box of 1e26
    # pixels.  A twentieth of their weights keeps w and h within a few anchors' sizes and the scores away from 0 and 1.
    with torch.no_grad():
        for i in model.yolo_layers:
            for p in model.module_list[i - 1].parameters():
                p.mul_(HEAD_GAIN)
    return model


def choose_threshold(M):
    """M [images, scales]: the largest score of each image at each scale.  -> the lowest midpoint between two score levels of M that
    leaves (a) an image without any detection, (b) another image with a scale without detections and a scale with some, (c) an image
    with detections at the middle scale, the one the single-scale tests run; None when there is none"""
    levels = np.unique(M)
    for lo, hi in zip(levels[:-1], levels[1:]):
        thr = float((lo + hi) / 2)
        has = M > thr
        if (~has.any(1)).any() and (has.any(1) & ~has.all(1)).any() and has[:, M.shape[1] // 2].any():
            return thr
    return None


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("detect_images")
    for name, a in zip(NAMES, make_images()):
        Image.fromarray(a).save(str(root / name))
    (root / 'notes.txt').write_text('not an image\n')
    return str(root)


@pytest.fixture(scope="module")
def model(cuda_dev):
    m = fill_procedural(Darknet(make_cfg.darknet53(), {"context_factor": 1.0}))
    return calibrate(m, make_images()).to(cuda_dev).eval()


@pytest.fixture(scope="module")
def loaded(folder, cuda_dev):
    """(paths, cache, shapes) of the one batch of five"""
    batches = list(ds.LoadImages(folder, S, 5, cuda_dev))
    assert len(batches) == 1
    paths, cache, shapes = batches[0]
    order = sorted(range(5), key=lambda k: NAMES[k])
    assert [os.path.basename(p) for p in paths] == [NAMES[k] for k in order] and list(shapes) == [SIZES[k] for k in order]
    assert cache.nbytes == sum(3 * h * w for h, w in SIZES)          # the original pixels, nothing resized
    return paths, cache, shapes


@pytest.fixture(scope="module")
def thr(model, loaded, cuda_dev):
    _, cache, shapes = loaded
    M = np.zeros((5, len(SCALES)))
    with torch.no_grad():
        for k, size in enumerate(SCALES):
            io = model(ds.letterbox_batch(cache, shapes, size))[0].float()
            ok = (io[..., 2:4] > 2).all(2) & torch.isfinite(io).all(2)
            M[:, k] = torch.where(ok, io[..., 5] * io[..., 6], torch.zeros((), device=cuda_dev)).max(1).values.cpu().numpy()
    t = choose_threshold(M)
    print("largest score per image and scale:\n%s\nthreshold %r" % (M, t))
    assert t is not None, "no score level separates the images as the tests need:\n%s" % M
    return t


def make_opt(model, monkeypatch, cuda_dev, **kw):
    monkeypatch.setattr(detect, 'Darknet', lambda cfg, hyp: model)          # the procedural model, not a freshly initialised one
    opt = argparse.Namespace(hyp='', cfg='procedural', weights='', source='', output='', img_size=S, conf_thres=0.5, nms_thres=NMS,
                             batch_size=5, synthetic=5, torch_device=cuda_dev, multi_scale=False, scales='', seed=0, icdar=False)
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def row_text(rows):
    return ''.join(('%g ' * 7 + '\n') % (*box, conf, cls) for *box, conf, _, cls in rows)


def files_of(folder):
    return {n: open(os.path.join(folder, n)).read() for n in sorted(os.listdir(folder)) if n.endswith('.txt')}


def expected_single_scale(model, loaded, thr):
    """per image the fp32 rows the composition gives: letterbox_area + model.detect on the GPU, the numpy rescale on the CPU"""
    paths, cache, shapes = loaded
    with torch.no_grad():
        out = model.detect(ds.letterbox_batch(cache, shapes, S), thr, NMS)
    geom = rescale_geometry(shapes, S)
    rows = []
    for k, o in enumerate(out):
        o = np.zeros((0, 8), dtype=np.float32) if o is None else o.cpu().numpy()
        rows.append(dref.rescale(o, [0, len(o)], geom[k:k + 1]))
    return rows


def test_single_scale_files_icdar_rows_and_zip(cuda_dev, model, loaded, thr, folder, tmp_path, monkeypatch):
    paths = loaded[0]
    want = expected_single_scale(model, loaded, thr)
    counts = [len(r) for r in want]
    print("detections per image at %d: %s" % (S, counts))
    assert min(counts) == 0 and max(counts) > 0
    out = str(tmp_path / 'out')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=folder, output=out, conf_thres=thr, icdar=True))
    got = files_of(out)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    assert sorted(got) == sorted(s + '.txt' for s in stems)
    for s, rows in zip(stems, want):
        assert got[s + '.txt'] == row_text(rows.tolist()), s
    icdar = files_of(os.path.join(out, 'icdar'))
    assert sorted(icdar) == sorted(icdar_name(p) for p in paths)
    texts = {}
    for p, rows in zip(paths, want):
        q, xy = dref.quads(rows)
        assert dref.comparable(rows).all(), "a corner within 1e-6 of an integer: choose other pictures"
        texts[icdar_name(p)] = ''.join(','.join('%d' % v for v in r) + '\n' for r in q.tolist())
        assert icdar[icdar_name(p)] == texts[icdar_name(p)], p
    with zipfile.ZipFile(os.path.join(out, 'icdar_result.zip')) as zf:
        assert zf.namelist() == sorted(texts)
        for name in zf.namelist():
            assert zf.read(name).decode() == texts[name]


def test_batch_size_two_pads_the_last_batch_and_gives_the_same_files(cuda_dev, model, thr, folder, tmp_path, monkeypatch):
    outs = {}
    for bs in (5, 2):
        outs[bs] = str(tmp_path / ('bs%d' % bs))
        detect.detect(make_opt(model, monkeypatch, cuda_dev, source=folder, output=outs[bs], conf_thres=thr, batch_size=bs, icdar=True))
    assert files_of(outs[2]) == files_of(outs[5]) and len(files_of(outs[5])) == 5
    assert files_of(os.path.join(outs[2], 'icdar')) == files_of(os.path.join(outs[5], 'icdar'))
    assert any(files_of(outs[5]).values())


def test_one_file_and_a_list_are_sources_too(cuda_dev, model, thr, folder, tmp_path, monkeypatch):
    whole = str(tmp_path / 'whole')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=folder, output=whole, conf_thres=thr))
    lst = tmp_path / 'list.txt'
    lst.write_text('\n'.join(os.path.join(folder, n) for n in (NAMES[0], NAMES[3])) + '\n')
    part = str(tmp_path / 'part')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=str(lst), output=part, conf_thres=thr))
    one = str(tmp_path / 'one')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=os.path.join(folder, NAMES[1]), output=one, conf_thres=thr))
    w = files_of(whole)
    assert files_of(part) == {k: w[k] for k in ('b_square.txt', 'e_wide.txt')} and files_of(one) == {'a_tall.txt': w['a_tall.txt']}


def test_a_second_run_into_the_same_folder_zips_its_own_files_only(cuda_dev, model, thr, folder, tmp_path, monkeypatch):
    out = str(tmp_path / 'out')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=folder, output=out, conf_thres=thr, icdar=True))
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=os.path.join(folder, NAMES[3]), output=out, conf_thres=thr, icdar=True))
    assert len(files_of(os.path.join(out, 'icdar'))) == 5                 # the first run's files are still there
    with zipfile.ZipFile(os.path.join(out, 'icdar_result.zip')) as zf:
        assert zf.namelist() == ['res_b_square.txt']


def test_two_images_with_one_stem_are_refused(cuda_dev, model, thr, folder, tmp_path, monkeypatch):
    from PIL import Image
    d = tmp_path / 'twins'
    d.mkdir()
    for name in ('a.png', 'a.bmp'):
        Image.fromarray(make_images()[2]).save(str(d / name))
    with pytest.raises(ValueError, match="stem"):
        detect.detect(make_opt(model, monkeypatch, cuda_dev, source=str(d), output=str(tmp_path / 'out'), conf_thres=thr))


def test_video_sources_are_refused_not_replaced_by_synthetic_images(cuda_dev, model, tmp_path, monkeypatch):
    clip = tmp_path / 'clip.mp4'
    clip.write_bytes(b'x')
    for source in (str(clip), '0'):
        with pytest.raises(NotImplementedError, match="OpenCV"):
            detect.detect(make_opt(model, monkeypatch, cuda_dev, source=source, output=str(tmp_path / 'out')))


def test_multi_scale_equals_the_reference_flow_on_the_cpu(cuda_dev, model, loaded, thr):
    paths, cache, shapes = loaded
    out, det, det_off = detect_images(model, cache, 5, shapes, SCALES, thr, NMS)
    # the reference: per scale NMS at 0.95, scale_coords().round(), concatenate, one more non_max_suppression -- on the same per-scale rows
    per_image = [[] for _ in range(5)]
    none_at_a_scale = set()
    with torch.no_grad():
        for size in SCALES:
            geom = rescale_geometry(shapes, size)
            for k, o in enumerate(model.detect(ds.letterbox_batch(cache, shapes, size), thr, 0.95)):
                if o is None:
                    none_at_a_scale.add(k)
                else:
                    per_image[k].append(torch.from_numpy(dref.rescale(o.cpu().numpy(), [0, len(o)], geom[k:k + 1])))
    empty = [k for k in range(5) if not per_image[k]]
    print("rows per image and scale: %s" % [[len(r) for r in rows] for rows in per_image])
    assert empty and (none_at_a_scale - set(empty)), "the threshold must leave an image without detections and one without at one scale"
    off = det_off.cpu().tolist()
    assert off[0] == 0 and off[5] == len(det)
    for k in range(5):
        want = do.non_max_suppression(torch.cat(per_image[k]).unsqueeze(0), thr, NMS)[0] if per_image[k] else None
        assert (out[k] is None) == (want is None), k
        assert off[k + 1] - off[k] == (0 if want is None else len(want))
        if want is not None:
            assert torch.equal(out[k].cpu(), want), k
            assert torch.equal(det[off[k]:off[k + 1]].cpu(), want)
    assert any(o is not None for o in out)


def test_multi_scale_through_detect_py(cuda_dev, model, loaded, thr, folder, tmp_path, monkeypatch, capsys):
    paths, cache, shapes = loaded
    out = str(tmp_path / 'ms')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=folder, output=out, conf_thres=thr, multi_scale=True, scales='64,96,128'))
    assert 'use scale: [64, 96, 128]' in capsys.readouterr().out
    rows, _, _ = detect_images(model, cache, 5, shapes, SCALES, thr, NMS)
    got = files_of(out)
    for p, r in zip(paths, rows):
        stem = os.path.splitext(os.path.basename(p))[0]
        assert got[stem + '.txt'] == row_text([] if r is None else r.cpu().tolist())


def _old_tensor_mode_files(model, imgs, thr, cuda_dev):
    """detect.py's tensor path as it was before the image path existed"""
    files = {}
    with torch.no_grad():
        for b in range(0, len(imgs), 5):
            for i, det in enumerate(model.detect(imgs[b:b + 5].to(cuda_dev), thr, NMS)):
                files['img_%d.txt' % (b + i)] = '' if det is None else row_text(det.cpu().tolist())
    return files


def test_npy_source_and_synthetic_fallback_are_unchanged(cuda_dev, model, thr, tmp_path, monkeypatch, capsys):
    x = torch.rand(5, 3, S, S, generator=torch.Generator().manual_seed(3))
    np.save(str(tmp_path / 'x.npy'), x.numpy())
    out = str(tmp_path / 'npy')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=str(tmp_path / 'x.npy'), output=out, conf_thres=thr))
    assert files_of(out) == _old_tensor_mode_files(model, x, thr, cuda_dev)
    out = str(tmp_path / 'syn')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=str(tmp_path / 'no_such_folder'), output=out, conf_thres=thr))
    syn = torch.rand(5, 3, S, S, generator=torch.Generator().manual_seed(0))
    assert files_of(out) == _old_tensor_mode_files(model, syn, thr, cuda_dev) and len(files_of(out)) == 5
    assert 'NOTE' not in capsys.readouterr().out
    # the flags of the image path say that they do nothing here, and do nothing
    out2 = str(tmp_path / 'syn_flags')
    detect.detect(make_opt(model, monkeypatch, cuda_dev, source=str(tmp_path / 'no_such_folder'), output=out2, conf_thres=thr,
                           multi_scale=True, scales='64,128', icdar=True))
    printed = capsys.readouterr().out
    assert 'NOTE: --multi-scale, --scales, --icdar: only for a --source of image files' in printed
    assert files_of(out2) == files_of(out) and sorted(os.listdir(out2)) == sorted(files_of(out2))
