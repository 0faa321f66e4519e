"""ctypes binding of include/ryolo.h (libryolo_hip.so).

The header is the only place a signature is written: importing this module parses it (no library needed) into `_sigs`,
entry point -> (restype, argtypes) for every prototype, and into the ctypes.Structure classes of its `typedef struct`s
(ConvDesc, PackJob, WgradReduceJob, SgdJob, AdamJob); lib() applies the whole table when it loads the library.  A type the parser
has no mapping for fails the import -- nothing is guessed, nothing is left to ctypes' default of passing a C int.

The library is built in-tree by __graft_entry__.build() (hipcc --offload-arch=gfx950).  There is NO fallback:
if the shared object is missing, or a call returns an error code, a RuntimeError is raised.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# RYOLO_HIP_LIB: another build of the same sources (the ablation build of tools/mp_ablate.py); never a different implementation
LIB_PATH = os.environ.get("RYOLO_HIP_LIB") or os.path.join(_HERE, "libryolo_hip.so")

_lib = None

ACT_LINEAR, ACT_LEAKY, ACT_MISH = 0, 1, 2

_SCALARS = {"int": C.c_int, "float": C.c_float, "long long": C.c_longlong, "size_t": C.c_size_t}
# what a pointer may point at; every pointer is passed as an address (c_void_p) but for the two exceptions in _ctype
_POINTEES = {"void", "char", "float", "double", "int", "unsigned", "unsigned char", "long long", "int32_t", "int64_t", "uint8_t", "uint64_t"}


def _ctype(decl, named, structs, where):
    """ctypes type of one C declarator of the header (`const float *const *ng`, `long long n`, `void`; named: it ends in an identifier)"""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    stars = words.count("*")
    base = " ".join(w for w in (words[:-1] if named else words) if w != "*")
    if not stars:
        if base in _SCALARS:
            return _SCALARS[base]
    elif base == "char" and stars == 1:
        return C.c_char_p
    elif base in structs:      # the descriptor is always a host struct, passed with byref; the job structs are device arrays too
        return C.POINTER(structs[base]) if base == "ryolo_conv_desc" and stars == 1 else C.c_void_p
    elif base in _POINTEES:
        return C.c_void_p
    raise RuntimeError("include/ryolo.h: %s: no ctypes mapping for `%s`" % (where, " ".join(decl.split())))


def _parse_header(text):
    """-> ({typedef name: ctypes.Structure class}, {entry point: (restype, argtypes)}) of the text of include/ryolo.h.  Handles the
    forms that header uses and raises on anything else: block comments, # lines, extern "C", `typedef struct` bodies of scalar, array and
    pointer fields, and prototypes over the closed type map above."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs, sigs = {}, {}

    def struct(m):
        body, name = m.group(1), m.group(2)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            where = "struct %s, field `%s`" % (name, decl)
            if "*" in decl:
                fields.append((decl.split("*")[-1].strip(), _ctype(decl, True, structs, where)))
                continue
            first = decl.split(",")[0].split()
            ctype = _ctype(" ".join(first), True, structs, where)
            for item in [first[-1]] + decl.split(",")[1:]:
                m2 = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", item)
                if not m2:
                    raise RuntimeError("include/ryolo.h: %s: not understood" % where)
                fields.append((m2.group(1), ctype * int(m2.group(2)) if m2.group(2) else ctype))
        cls = "".join(w.title() for w in name.split("_")[1:])      # ryolo_conv_desc -> ConvDesc
        structs[name] = type(cls, (C.Structure,), {"_fields_": fields, "__doc__": "%s of include/ryolo.h" % name})
        return ""

    def proto(m):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        where = "prototype %s" % name
        restype = None if ret.split() == ["void"] else _ctype(ret, False, structs, where)
        argtypes = [] if params == "void" else [_ctype(p, True, structs, where) for p in params.split(",")]
        sigs[name] = (restype, argtypes)
        return ""

    text = re.sub(r"typedef\s+struct\s+\w+\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*;", proto, text)
    rest = text.replace('extern "C" {', "", 1).replace("}", "", 1).strip()
    if rest:
        raise RuntimeError("include/ryolo.h: not understood: `%s`" % " ".join(rest.split())[:120])
    return structs, sigs


with open(os.path.join(_HERE, os.pardir, "include", "ryolo.h")) as _fh:
    _structs, _sigs = _parse_header(_fh.read())      # _sigs: entry point -> (restype, argtypes), every prototype of the header
ConvDesc, PackJob = _structs["ryolo_conv_desc"], _structs["ryolo_pack_job"]
WgradReduceJob, SgdJob = _structs["ryolo_wgrad_reduce_job"], _structs["ryolo_sgd_job"]
AdamJob = _structs["ryolo_adam_job"]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "rotate-yolov3_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP hot path." % LIB_PATH)
        # torch first: its bundled HIP runtime (libamdhip64) must be the one already in the process when the library's own
        # dependency on libamdhip64 is resolved -- loading this library BEFORE torch pulls in the system ROCm runtime and the
        # process ends up with two, streams and memory from one, kernels registered with the other: every launch then fails
        # (seen as `build(); smoke()` in one process: "HIP launch failed")
        import torch  # noqa: F401
        loaded = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _sigs.items():
            try:
                fn = getattr(loaded, name)
            except AttributeError:
                raise RuntimeError("rotate-yolov3_amd: include/ryolo.h declares %s but %s does not export it -- rebuild the "
                                   "library (__graft_entry__.build())" % (name, LIB_PATH))
            fn.restype, fn.argtypes = restype, argtypes
        _lib = loaded
    return _lib


TUNING_SWITCHES = ("RYOLO_CONV3X3", "RYOLO_CONV1X1", "RYOLO_RNMS_TILES", "RYOLO_MQ_KORDER", "RYOLO_BN_REDUCE_TILES", "RYOLO_STEM_DGRAD")


def set_tuning(name, value):
    """Set (value: str) or clear (None) one of the library's tuning switches in this process (include/ryolo.h: ryolo_set_tuning).  The
    library reads the environment only once, so tests and in-process A/Bs go through here."""
    rc = getattr(lib(), "_real", lib()).ryolo_set_tuning(name.encode(), None if value is None else str(value).encode())
    if rc != 0:
        raise RuntimeError("ryolo_set_tuning(%s): unknown switch" % name)


class _CallTracer(object):
    """Stands in for the CDLL while trace_calls() is active: every entry point called through lib() is bracketed by two events on
    torch's current stream and logged as (name, args, start, end).  Measurement plumbing for bench.py's in-run kernel tables; the
    product path never sees it."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("ryolo_") or not callable(fn):
            return fn
        log = self._log

        def traced(*args):
            import torch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            log.append((name, args, e0, e1))
            return rc
        return traced


class trace_calls(object):
    """with trace_calls() as log: ... -> log = [(entry point, ctypes args, start event, end event)] of every library call made inside
    (launches must be eager: a hipGraph replay makes no calls)."""

    def __enter__(self):
        global _lib
        lib()
        self._saved = _lib
        self.log = []
        _lib = _CallTracer(self._saved, self.log)
        return self.log

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved
        return False


def check(rc, what):
    if rc != 0:
        msg = lib().ryolo_strerror(rc)
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg.decode() if msg else "?", rc))


def stream_ptr(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream
