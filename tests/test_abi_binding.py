"""CPU tier: the ctypes binding (rotate-yolov3_amd/_lib.py) is derived from include/ryolo.h and from nothing else -- every prototype is
bound, the awkward ones map as written out here by hand, the derived structures have the layout the C compiler gives the header's, an
unknown type fails the parse, and no other file restates a signature the header declares."""
import ctypes as C
import os
import re
import subprocess

import pytest

import rotate_yolov3_amd  # noqa: F401
from rotate_yolov3_amd import _lib
from rotate_yolov3_amd.model import hip_ops, hip_train_ops
from rotate_yolov3_amd.utils import fused_sgd
from tests.test_cabi import ROOT, _binding, _declared

VP, I, F, LL, SZ = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t
STRUCTS = {"ryolo_conv_desc": _lib.ConvDesc, "ryolo_pack_job": hip_train_ops.PackJob,
           "ryolo_wgrad_reduce_job": hip_train_ops.WgradReduceJob, "ryolo_sgd_job": fused_sgd._Job}


def test_every_prototype_of_the_header_is_bound():
    names = _declared()
    assert len(names) >= 88 and sorted(_lib._sigs) == names
    lib = _binding()
    for n in names:
        fn = getattr(lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == _lib._sigs[n][1] and fn.restype is _lib._sigs[n][0], n


def test_the_awkward_prototypes_map_as_written_by_hand():
    s = _lib._sigs
    assert s["ryolo_build_id"] == (C.c_char_p, [])
    assert s["ryolo_rnms_count_pairs"] == (None, [VP])
    assert s["ryolo_rnms"] == (I, [VP, I, I, F, VP, VP, VP, SZ, VP])
    assert s["ryolo_build_targets"] == (I, [VP, VP, I, I, I, VP, VP, F, F, F, VP, VP, VP, VP, VP])
    assert s["ryolo_conv0_bn_bwd_workspace_bytes"] == (SZ, [])
    restype, args = s["ryolo_yolo_loss_nhwc_bias"]
    # the longest prototype, counted by hand in the header: 37 parameters, 7 of them float -- giou .. obj_pw in a row, then fl_gamma
    # behind iou_mode and arc
    assert restype is I and len(args) == 37 == max(len(a) for _, a in s.values())
    assert [k for k, t in enumerate(args) if t is F] == [20, 21, 22, 23, 24, 25, 28]
    assert [k for k, t in enumerate(args) if t is I] == [1, 3, 4, 5, 6, 7, 8, 10, 26, 27, 32, 35]
    assert all(t in (VP, I, F) for t in args)
    # the descriptor is the one typed pointer, and the classes are the objects the wrappers and bench.py use
    assert s["ryolo_conv2d_bn_act"][1][0] is C.POINTER(_lib.ConvDesc) and hip_ops.ConvDesc is _lib.ConvDesc
    assert s["ryolo_sgd_step"] == (I, [VP, I, I, VP, I, VP])


def test_structures_have_the_layout_the_c_compiler_gives_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include "ryolo.h"', 'int main(void) {']
    for cname, cls in sorted(STRUCTS.items()):
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field in cls._fields_:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field[0], cname, field[0]))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, what, value = ln.split()
        got[cname, what] = int(value)
    want = {}
    for cname, cls in STRUCTS.items():
        want[cname, "sizeof"] = C.sizeof(cls)
        for field in cls._fields_:
            want[cname, field[0]] = getattr(cls, field[0]).offset
    assert got == want
    # field counts: a field the parser dropped would be missing from both sides above
    assert [len(STRUCTS[k]._fields_) for k in sorted(STRUCTS)] == [15, 14, 8, 14]
    assert hip_train_ops.PackJob.khs.size == 36 and C.sizeof(hip_train_ops.WgradReduceJob) == 64


@pytest.mark.parametrize("proto,named", [
    ("int ryolo_new_thing(const float *x, double eps, void *stream);", "ryolo_new_thing"),
    ("int ryolo_new_thing(const float *x, short n);", "ryolo_new_thing"),
    ("double ryolo_new_value(void);", "ryolo_new_value"),
    ("int ryolo_new_thing(const strange_t *x);", "ryolo_new_thing"),
])
def test_a_type_outside_the_map_fails_the_parse_and_names_the_prototype(proto, named):
    good = "/* c */\n#define X 1\nextern \"C\" {\nint ryolo_fine(int a /* host */, long long b);\n%s\n}\n"
    structs, sigs = _lib._parse_header(good % "")
    assert sigs == {"ryolo_fine": (I, [I, LL])} and structs == {}
    with pytest.raises(RuntimeError, match=named):
        _lib._parse_header(good % proto)


def test_text_the_parser_does_not_understand_fails_the_parse():
    with pytest.raises(RuntimeError, match="not understood"):
        _lib._parse_header("int ryolo_fine(int a);\nstatic inline int ryolo_helper(int a) { return a; }\n")


def test_no_second_copy_of_a_declared_signature():
    declared = set(_declared())
    hits = []
    for top in ("rotate-yolov3_amd", "tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in sorted(files):
                path = os.path.join(dirpath, f)
                if not f.endswith(".py") or os.path.samefile(path, _lib.__file__):
                    continue
                txt = open(path, errors="ignore").read()
                for m in re.finditer(r"\b(ryolo_[a-z0-9_]+)\s*\.\s*(?:argtypes|restype)\b[^=\n]*=(?!=)|\bdeclare\(\s*[\"'](ryolo_[a-z0-9_]+)", txt):
                    if (m.group(1) or m.group(2)) in declared:
                        hits.append("%s: %s" % (os.path.relpath(path, ROOT), m.group(0)))
    assert not hits, hits
