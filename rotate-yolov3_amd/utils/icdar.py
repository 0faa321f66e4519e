"""The ICDAR result files of the reference's detect.py (utils/ICDAR/icdar_utils.py: xywha2icdar, zip_dir): per image one
res_<stem>.txt with a line x0,y0,x1,y1,x2,y2,x3,y3 per detection (tl, tr, br, bl as hip_ops.det_quads orders them), and the folder
zipped with the file names as archive names, which is what the ICDAR evaluation server takes."""
import os
import zipfile


def icdar_name(img_path):
    return 'res_%s.txt' % os.path.splitext(os.path.basename(img_path))[0]


def write_icdar(folder, img_path, quads):
    """res_<stem>.txt of one image in `folder`: `quads` is a sequence of 8 integers per detection (none: an empty file).  Returns the path."""
    path = os.path.join(folder, icdar_name(img_path))
    with open(path, 'w') as f:
        for q in quads:
            q = [int(v) for v in q]
            if len(q) != 8:
                raise ValueError('an ICDAR row has 8 coordinates, not %d' % len(q))
            f.write(','.join('%d' % v for v in q) + '\n')
    return path


def zip_files(files, zipfilename):
    """the given files into a deflated zip, named by their base names, in sorted order: the result files of ONE run, whatever else lies
    in their folder"""
    names = [os.path.basename(f) for f in files]
    if len(set(names)) != len(names):
        raise ValueError('zip_files: two files share a name')
    with zipfile.ZipFile(zipfilename, 'w', zipfile.ZIP_DEFLATED) as zf:
        for arc, full in sorted(zip(names, files)):
            zf.write(full, arc)
    return zipfilename


def zip_dir(dirname, zipfilename):
    """every file under `dirname` (or the file itself) into a deflated zip, in sorted order, named by its path below `dirname`"""
    if os.path.isfile(dirname):
        files = [(dirname, os.path.basename(dirname))]
    else:
        files = []
        for root, _, names in os.walk(dirname):
            for name in names:
                full = os.path.join(root, name)
                files.append((full, os.path.relpath(full, dirname)))
    with zipfile.ZipFile(zipfilename, 'w', zipfile.ZIP_DEFLATED) as zf:
        for full, arc in sorted(files, key=lambda t: t[1]):
            zf.write(full, arc)
    return zipfilename
