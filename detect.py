#!/usr/bin/env python
"""detect.py -- inference entry point mirroring the reference's detect.py (detect() :142-275, multi_detect() :16-137, flags :279-296):
load cfg (+ .pt / darknet .weights), forward on the HIP engine, rotated NMS, write one text row per detection
(x y w h angle score class).

--source is
  * a directory of images, one image file or a .txt list of image paths: Pillow decodes, the original pixels go to the GPU once per
    batch, ryolo_letterbox_area writes the letterboxed batch at the network size, and the rows are scaled back to the original image
    (scale_coords(...).round()) on the device.  Per image: <output>/<stem>.txt.  --icdar adds <output>/icdar/res_<stem>.txt
    (x0,y0,..,x3,y3 per detection) and <output>/icdar_result.zip of them.  --multi-scale runs every image at several sizes (--scales, or
    two sizes drawn from the reference's range with --seed) and merges the rows with one more rotated NMS (multi_detect).
    The zip holds the files of this run only; two images with the same stem are refused.
    --save-img adds the picture itself, <output>/<name of the image file>, with every detection drawn into it as the reference's
    plot_one_box does: the rotated outline (ryolo_det_corners + ryolo_draw_quads on the original pixels, on the device; thickness
    round(0.002 (h + w) / 2) + 1 or --line-thickness) and the label '<class name> <score>' at the box's first corner, in the class's colour.
    The class names come from the `names` file of --data.  One download per batch; the files are encoded by a pool of threads (PNG stays
    PNG, JPEG at quality 95).  An --output that is the folder an image is read from is refused: the pictures would overwrite their sources.
  * a .npy / .pt tensor file [n,3,H,W] in [0,1], or anything that does not exist (`--synthetic N` random images): the tensor goes to
    the model as it is and the rows (network coordinates) to <output>/img_%d.txt.  --multi-scale, --scales, --seed, --icdar, --save-img and
    --line-thickness have no effect there and a NOTE says so.
  * the exception to "anything that does not exist": a camera number (`0`), a stream URL (rtsp:// rtmp:// http:// https://) or a video
    file that exists.  The reference opens these with OpenCV; here they are refused with a clear error instead of falling back to
    synthetic images.
--nms-style MERGE (all three kinds of source; default OR, the greedy NMS): every kept box becomes the score-weighted mean of the boxes it
suppresses (utils/nms/nms.py).  With several sizes that happens in the merge over the scales, where one object gives one estimate per size.
The outline is this port's own exact definition (include/ryolo.h: ryolo_draw_quads), not cv2.polylines pixel for pixel; the label is
upright.  Displaying the pictures (--view-img) and video output are out of scope."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import rotate_yolov3_amd  # noqa: E402,F401
from rotate_yolov3_amd.model.model_utils import load_darknet_weights  # noqa: E402
from rotate_yolov3_amd.model.models import Darknet  # noqa: E402
from rotate_yolov3_amd.utils.parse_config import hyp_parse  # noqa: E402


def multi_scale_sizes(img_size, seed=0, size_num=2):
    """the reference's draw (detect.py:55-58): size_num different multiples of 32 from
    [(round(img_size / 32 / 1.5) + 1) * 32, (round(img_size / 32 * 1.3) - 1) * 32], here from a numpy Generator seeded by `seed`"""
    lo, hi = multi_scale_range(img_size)
    return [int(x) for x in np.random.default_rng(int(seed)).choice(np.arange(lo, hi + 32, 32), size_num, replace=False)]


def multi_scale_range(img_size):
    """(smallest, largest) size --multi-scale draws from"""
    return (round(img_size / 32 / 1.5) + 1) * 32, (round(img_size / 32 * 1.3) - 1) * 32


def parse_scales(text):
    """'416,608,800' -> [416, 608, 800]: positive multiples of 32, no repeats"""
    try:
        sizes = [int(s) for s in str(text).split(',') if s.strip() != '']
    except ValueError:
        raise ValueError('--scales %r: a comma separated list of integers' % text)
    if not sizes or any(s < 32 or s % 32 for s in sizes) or len(set(sizes)) != len(sizes):
        raise ValueError('--scales %r: one or more different positive multiples of 32' % text)
    return sizes


def is_image_source(source):
    """a directory, an image file or a .txt list that exists -- and a camera number, a stream URL or a video file that exists, which
    LoadImages refuses with a clear error; tensor files and other paths that do not exist keep their old meaning"""
    from rotate_yolov3_amd.utils.datasets import IMG_FORMATS, VID_FORMATS, is_video_or_stream
    ext = os.path.splitext(source)[-1].lower()
    if ext in ('.npy', '.pt'):
        return False
    if is_video_or_stream(source):       # a camera number, a URL, a video file that exists: LoadImages gives the clear error
        return ext not in VID_FORMATS or os.path.isfile(source)
    return os.path.isdir(source) or (os.path.isfile(source) and (ext in IMG_FORMATS or ext == '.txt'))


def check_save_img_output(opt):
    """--save-img writes <output>/<name of the image file>: refuse an output folder that an image would be read from"""
    from rotate_yolov3_amd.utils.datasets import list_images
    out = os.path.realpath(opt.output)
    for p in list_images(opt.source):
        if os.path.realpath(os.path.dirname(os.path.abspath(p))) == out:
            raise ValueError('detect.py --save-img: --output %r is the folder %r is read from: the drawn pictures would overwrite their '
                             'sources; choose another --output' % (opt.output, p))


def class_names(opt):
    """the class names of --data for the labels; without the files a NOTE, and the labels carry class indices"""
    from rotate_yolov3_amd.utils.plots import load_class_names
    data = getattr(opt, 'data', '')
    names = load_class_names(data)
    if names is None:
        print('NOTE: --data %r: no *.data file with a `names` file there: the labels carry class indices' % data)
    return names


def detect_image_files(model, opt, device):
    """the image path: LoadImages -> detect_images per batch -> <stem>.txt (+ ICDAR rows, + the drawn pictures); returns (images, detections)"""
    from rotate_yolov3_amd.model import hip_ops
    from rotate_yolov3_amd.utils.datasets import LoadImages
    from rotate_yolov3_amd.utils.detect_images import detect_images
    from rotate_yolov3_amd.utils.icdar import write_icdar, zip_files
    sizes = [opt.img_size]
    if getattr(opt, 'scales', ''):
        sizes = parse_scales(opt.scales)
    elif getattr(opt, 'multi_scale', False):
        sizes = multi_scale_sizes(opt.img_size, getattr(opt, 'seed', 0))
    if len(sizes) > 1 or getattr(opt, 'multi_scale', False):
        print('use scale: {}'.format(sizes))
    icdar = getattr(opt, 'icdar', False)
    icdar_dir = os.path.join(opt.output, 'icdar')
    if icdar:
        os.makedirs(icdar_dir, exist_ok=True)
    dataset = LoadImages(opt.source, opt.img_size, opt.batch_size, device)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in dataset.files]
    twice = sorted(set(s for s in stems if stems.count(s) > 1))
    if twice:
        raise ValueError('detect.py: the result files are named by the image\'s stem, and %d stems occur more than once (%s ...): '
                         'their results would overwrite each other' % (len(twice), twice[0]))
    save_img = getattr(opt, 'save_img', False)
    if save_img:
        from concurrent.futures import ThreadPoolExecutor
        from rotate_yolov3_amd.utils import plots
        names = class_names(opt)
        colors = plots.class_colors(len(names) if names else plots.DEFAULT_CLASSES)
        thick = int(getattr(opt, 'line_thickness', 0) or 0) or None
        pool = ThreadPoolExecutor(max_workers=max(1, min(8, opt.batch_size, os.cpu_count() or 1)))
        pending = []                     # the encodings in flight, a list per batch: at most two batches' pixels are held
    n_img = n_det = 0
    icdar_files = []
    for paths, cache, shapes in dataset:
        n = len(paths)
        out, det, det_off = detect_images(model, cache, n, shapes, sizes, opt.conf_thres, opt.nms_thres, slots=opt.batch_size,
                                          nms_style=getattr(opt, 'nms_style', 'OR'))
        quads = hip_ops.det_quads(det).cpu().tolist() if icdar else None
        off = det_off.cpu().tolist()
        rows = det.cpu().tolist()
        for i, p in enumerate(paths):
            stem = os.path.splitext(os.path.basename(p))[0]
            with open(os.path.join(opt.output, stem + '.txt'), 'w') as f:
                for *box, conf, _, cls in rows[off[i]:off[i + 1]]:
                    f.write(('%g ' * 7 + '\n') % (*box, conf, cls))
            if icdar:
                icdar_files.append(write_icdar(icdar_dir, p, quads[off[i]:off[i + 1]]))
        if save_img:
            # the boxes and labels are painted on the device; ONE download of the batch's pixels, the encoders work on views of it
            drawn = plots.draw_detections(cache, n, det, det_off, names, colors, thick, host_rows=rows).cpu().numpy()
            while len(pending) > 1:
                for f in pending.pop(0):
                    f.result()           # an encoder's error is the run's error
            pending.append([])
            at = 0
            for p, (h, w) in zip(paths, cache.hw):
                pending[-1].append(pool.submit(plots.save_image, drawn[at:at + 3 * h * w].reshape(h, w, 3),
                                               os.path.join(opt.output, os.path.basename(p))))
                at += 3 * h * w
        n_img += n
        n_det += off[n]
    if save_img:
        pool.shutdown(wait=True)
        for batch in pending:
            for f in batch:
                f.result()
    if icdar:
        # the files of this run only: the folder may hold res_*.txt of an earlier run with other images
        zip_files(icdar_files, os.path.join(opt.output, 'icdar_result.zip'))
    return n_img, n_det


def detect(opt):
    if getattr(opt, 'save_img', False) and is_image_source(opt.source):
        check_save_img_output(opt)       # before anything is loaded or written
    from rotate_yolov3_amd.utils.nms.nms import check_nms_style
    check_nms_style(getattr(opt, 'nms_style', 'OR'))
    device = getattr(opt, 'torch_device', None) or torch.device('cuda:0')
    hyp = hyp_parse(opt.hyp) if opt.hyp and os.path.isfile(opt.hyp) else {'context_factor': 1.0}
    model = Darknet(opt.cfg, hyp)
    if opt.weights and not os.path.isfile(opt.weights):
        print('NOTE: weights file %r not found: running the freshly initialised model' % opt.weights)
    elif opt.weights.endswith('.pt'):
        model.load_state_dict(torch.load(opt.weights, map_location='cpu')['model'])
    elif opt.weights:
        load_darknet_weights(model, opt.weights)
    model.to(device).eval()
    if is_image_source(opt.source):
        os.makedirs(opt.output, exist_ok=True)
        t0 = time.time()
        n_img, n_det = detect_image_files(model, opt, device)
        print('Done. %d images, %d detections (%.3fs)' % (n_img, n_det, time.time() - t0))
        return
    if opt.source.endswith('.npy'):
        imgs = torch.from_numpy(np.load(opt.source)).float()
    elif opt.source.endswith('.pt'):
        imgs = torch.load(opt.source).float()
    else:
        imgs = torch.rand(opt.synthetic, 3, opt.img_size, opt.img_size, generator=torch.Generator().manual_seed(0))
    given = [f for f, on in (('--multi-scale', getattr(opt, 'multi_scale', False)), ('--scales', getattr(opt, 'scales', '')),
                             ('--seed', getattr(opt, 'seed', 0)), ('--icdar', getattr(opt, 'icdar', False)),
                             ('--save-img', getattr(opt, 'save_img', False)), ('--line-thickness', getattr(opt, 'line_thickness', 0))) if on]
    if given:
        print('NOTE: %s: only for a --source of image files (a directory, an image, a .txt list); no effect on %r'
              % (', '.join(given), opt.source))
    os.makedirs(opt.output, exist_ok=True)
    t0 = time.time()
    n_det = 0
    style = {} if getattr(opt, 'nms_style', 'OR') == 'OR' else {'nms_style': opt.nms_style}
    with torch.no_grad():
        for b in range(0, len(imgs), opt.batch_size):
            # forward + non_max_suppression(pred, conf, nms) of the reference (detect.py:91-99), fused on the GPU
            for i, det in enumerate(model.detect(imgs[b:b + opt.batch_size].to(device), opt.conf_thres, opt.nms_thres, **style)):
                with open(os.path.join(opt.output, 'img_%d.txt' % (b + i)), 'w') as f:
                    if det is not None:
                        n_det += len(det)
                        for *box, conf, _, cls in det.cpu().tolist():
                            f.write(('%g ' * 7 + '\n') % (*box, conf, cls))
    print('Done. %d images, %d detections (%.3fs)' % (len(imgs), n_det, time.time() - t0))


def build_parser():
    """-> (parser, names of the flags that are accepted and ignored)"""
    from rotate_yolov3_amd.utils.cli import add_ignored
    parser = argparse.ArgumentParser()                                   # the reference's flags (detect.py:280-295), same defaults
    parser.add_argument('--hyp', type=str, default='cfg/ICDAR/hyp.py', help='hyper-parameter path')
    parser.add_argument('--cfg', type=str, default='cfg/ICDAR/yolov3_608_dh_o8_ga.cfg', help='cfg file path')
    parser.add_argument('--weights', type=str, default='weights/last.pt', help='path to weights file (.pt or darknet .weights)')
    parser.add_argument('--source', type=str, default='data/tiny/test', help='a directory of images, an image file, a .txt list of image paths, or a .npy / .pt tensor file [n,3,H,W] in [0,1]; a path that does not exist: --synthetic random images')
    parser.add_argument('--output', type=str, default='output', help='output folder')
    parser.add_argument('--img-size', type=int, default=608, help='inference size (pixels)')
    parser.add_argument('--conf-thres', type=float, default=0.5, help='object confidence threshold')
    parser.add_argument('--nms-thres', type=float, default=0.3, help='iou threshold for non-maximum suppression')
    parser.add_argument('--device', default='', help='device id (i.e. 0 or 0,1); the detection path has no CPU fallback')
    parser.add_argument('--batch-size', type=int, default=8, help='images per forward')
    parser.add_argument('--synthetic', type=int, default=8, help='random images when --source does not exist')
    parser.add_argument('--multi-scale', action='store_true', help='multi-scale testing of image files: every image at several sizes, merged by one more rotated NMS')
    parser.add_argument('--scales', type=str, default='', help='the sizes of multi-scale testing, e.g. 416,608,800 (multiples of 32); without it --multi-scale draws two sizes')
    parser.add_argument('--seed', type=int, default=0, help='seed of the --multi-scale size draw')
    parser.add_argument('--icdar', action='store_true', help='also write <output>/icdar/res_<stem>.txt and <output>/icdar_result.zip')
    parser.add_argument('--save-img', action='store_true', help='image files only: also write <output>/<image name>, the picture with the boxes and labels drawn in (on the device)')
    parser.add_argument('--line-thickness', type=int, default=0, help='outline thickness of --save-img in pixels, 1..255 (0: round(0.002 (h + w) / 2) + 1 per image)')
    parser.add_argument('--nms-style', type=str, default='OR', choices=['OR', 'MERGE'], help='OR: greedy rotated NMS; MERGE: every kept box becomes the score-weighted mean of the boxes it suppresses (with several scales: in the merge over the scales)')
    ignored = add_ignored(parser, [
        ('--data', dict(type=str, default='data/tiny.data', help='*.data file path: with --save-img its `names` file names the classes in the labels')),
        ('--fourcc', dict(type=str, default='mp4v', help='output video codec')),
        ('--half', dict(action='store_true', help='half precision FP16 inference (the HIP engine always computes in bf16 with fp32 accumulation)')),
        ('--view-img', dict(action='store_true', help='display results'))])
    return parser, ignored


if __name__ == '__main__':
    from rotate_yolov3_amd.utils.cli import pick_device, report_ignored
    parser, ignored = build_parser()
    opt = parser.parse_args()
    print(opt)
    report_ignored(parser, opt, [n for n in ignored if not (n == 'data' and opt.save_img)])     # --save-img reads --data
    if not 0 <= opt.line_thickness <= 255:
        parser.error('--line-thickness %d: 1..255, or 0 for the default' % opt.line_thickness)
    opt.torch_device = pick_device(opt.device)
    if opt.torch_device.type != 'cuda':
        sys.exit('detect.py: the detection path (HIP forward + rotated NMS) needs a GPU; --device %r selects none' % opt.device)
    detect(opt)
