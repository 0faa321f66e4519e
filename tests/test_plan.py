"""CPU tier: the layer planner (rotate-yolov3_amd/model/plan.py) over every point of the dispatch census (5 configs x 13 sizes x 7 batches).
The planner allocates nothing, so what the engines would build is checked here without a GPU: a plan builds or is refused with a known
message, concat buffers are tiled exactly by their homed slices and run-time copies, no launch reads what nobody wrote, and every
gradient view of the training plan has exactly one first writer."""
import re

import pytest

from tests import dispatch_census as dc
from rotate_yolov3_amd.model import plan

REFUSALS = [re.compile(p) for p in (
    r"conv \d+: channel counts must be multiples of 8 for the HIP path$",
    r"route \d+ joins tensors of different spatial size \(reorg is out of scope\)$",
    r"shortcut \d+ adds tensors of different shape$",
    r"training path: only x2 upsampling$",
    r"training path: maxpool graphs \(yolov3-tiny\) cannot train in the reference either \(model/loss.py:248 hard-codes three heads\)$",
    r"training path: route \d+ needs a copy \(unsupported graph\)$")]


def _plans(kind, nc, H, W, N):
    """(eval plan, train plan) of a census point; a refused one is None (the message must be a known one)"""
    defs = dc.config_defs(kind, nc, H, W)
    yolos = dc._yolos(defs)
    out = []
    for build in (lambda: plan.plan_eval(defs, dc._convs(defs), yolos, N, H, W), lambda: plan.plan_train(defs, dc._convs(defs), N, H, W)):
        try:
            out.append(build())
        except plan.Refused as e:
            assert any(p.match(str(e)) for p in REFUSALS), str(e)
            out.append(None)
    return defs, out[0], out[1]


def _chans(v):
    return set(range(v.off, v.off + v.C))


class _Written(object):
    """channels written so far, per buffer"""

    def __init__(self):
        self.w = {}

    def covers(self, v):
        return _chans(v) <= self.w.get(v.buf, set())

    def touches(self, v):
        return bool(_chans(v) & self.w.get(v.buf, set()))

    def write(self, v):
        self.w.setdefault(v.buf, set()).update(_chans(v))


def _check_concat(defs, buffers, views, copies, what):
    """the slices homed in a multi-input route's buffer are disjoint and 8-channel aligned and, with the copies, cover it exactly"""
    n = 0
    for i, d in enumerate(defs):
        if d["type"] != "route" or "," not in d["layers"]:
            continue
        whole = views[i]
        assert (whole.off, whole.C, whole.cs) == (0, buffers[whole.buf][0], buffers[whole.buf][0]), (what, i)
        homes = set(v for v in views if v is not None and v.buf == whole.buf and v != whole)
        seen = []
        for v in homes:
            assert v.off % 8 == 0 and v.C % 8 == 0 and (v.H, v.W, v.cs) == (whole.H, whole.W, whole.C), (what, i, v)
        for v in list(homes) + [c for c in copies if c.buf == whole.buf]:
            seen += list(_chans(v))
        assert sorted(seen) == list(range(whole.C)), (what, i, sorted(homes))
        n += 1
    return n


def _check_eval(defs, ep):
    assert _check_concat(defs, ep.buffers, ep.views, [op["out"] for op in ep.ops if op["kind"] == "copy"], "eval") >= 1
    done = _Written()
    done.write(ep.x)
    for op in ep.ops:
        for key in ("xin", "res", "a", "b"):
            v = op.get(key)
            assert v is None or done.covers(v), ("read before written", op["kind"], op["layer"], key, v)
        assert op["kind"] in ("head", "decode") or op["out"] is not None, op
        if op.get("out") is not None:
            c, h, w = ep.buffers[op["out"].buf]
            assert op["out"].off + op["out"].C <= c and (op["out"].H, op["out"].W, op["out"].cs) == (h, w, c), op
            done.write(op["out"])
    kinds = [op["kind"] for op in ep.ops]
    assert kinds.count("head") + kinds.count("decode") == sum(d["type"] == "yolo" for d in defs)
    for i, v in enumerate(ep.views):                          # a layer's view is something a launch has written
        assert v is None or done.covers(v), (i, v)


def _check_train(defs, tp):
    for views, what in ((tp.act, "act"), (tp.grd, "grd")):
        assert _check_concat(defs, tp.buffers, views, [], what) >= 1
    done = _Written()
    done.write(tp.x)
    for kind, i, pl in tp.forward:
        reads, out = {"conv": lambda: ([pl["xin"], pl["res"]], pl["y"]), "add": lambda: (pl[:2], pl[2]), "up": lambda: (pl[:1], pl[1]),
                      "yolo": lambda: (pl[:1], None)}[kind]()
        assert all(v is None or done.covers(v) for v in reads), ("read before written", kind, i)
        if out is not None:
            done.write(out)
    # backward: an entry flagged FIRST writes channels nobody wrote (it overwrites), any other accumulates onto channels that are all
    # initialised; every gradient an entry reads has been written -- so each gradient view that is read has exactly one first writer
    assert [(k, i) for k, i, _ in tp.backward] == [(k, i) for k, i, _ in reversed(tp.forward)]
    grads = _Written()

    def write(v, first, who):
        if first:
            assert not grads.touches(v), ("a second first writer", who, v)
            grads.write(v)
        else:
            assert grads.covers(v), ("accumulates onto an uninitialised gradient", who, v)

    for (kind, i, pl), (_, _, flags) in zip(reversed(tp.forward), tp.backward):
        if kind == "yolo":
            write(pl[1], True, (kind, i))                         # the loss writes the head gradient
            continue
        dy = pl["dy"] if kind == "conv" else (pl[5] if kind == "add" else pl[3])
        assert grads.covers(dy), ("reads a gradient nobody wrote", kind, i, dy)
        if kind == "conv":
            assert (flags[0] is None) == (pl["res_g"] is None or pl["res_alias"]) and (flags[1] is None) == (pl["xin_g"] is None)
            if flags[0] is not None:
                write(pl["res_g"], flags[0], (kind, i, "res_g"))
            if flags[1] is not None:
                write(pl["xin_g"], flags[1], (kind, i, "xin_g"))
            if pl["res_alias"]:
                assert pl["res_g"] == pl["dy"]
        elif kind == "add":
            write(pl[3], flags[0], (kind, i, "a_g"))
            write(pl[4], flags[1], (kind, i, "b_g"))
        else:
            write(pl[2], flags, (kind, i))


@pytest.mark.parametrize("kind,nc", dc.CONFIGS)
def test_every_census_point_plans_soundly_or_is_refused(kind, nc):
    planned = refused = 0
    for (H, W) in dc.SIZES:
        for N in dc.BATCHES:
            defs, ep, tp = _plans(kind, nc, H, W, N)
            if ep is not None:
                _check_eval(defs, ep)
            if tp is not None:
                _check_train(defs, tp)
            planned += (ep is not None) + (tp is not None)
            refused += (ep is None) + (tp is None)
    # Darknet-53 plans in both engines; yolov3-tiny has maxpool layers (no training) and, with one class, 252-channel heads (no inference)
    want = {"darknet53": (2, 0), "tiny": (1, 1) if nc != 1 else (0, 2)}[kind]
    assert (planned, refused) == tuple(k * len(dc.SIZES) * len(dc.BATCHES) for k in want)


def test_the_switches_are_arguments_and_the_planner_imports_no_torch():
    defs = dc.config_defs("darknet53", 1, 416, 416)
    kinds = lambda **kw: [op["kind"] for op in plan.plan_eval(defs, dc._convs(defs), dc._yolos(defs), 2, 416, 416, **kw).ops]      # noqa: E731
    on, off = kinds(), kinds(stem_pair=False, head_decode=False)
    assert on.count("pair") >= 1 and on.count("head") == 3 and "decode" not in on
    # a pair is one launch for two convs, a fused head one launch for conv + decode
    assert "pair" not in off and "head" not in off and off.count("decode") == 3 and len(off) == len(on) + on.count("pair") + 3
    b0 = plan.plan_train(defs, dc._convs(defs), 2, 416, 416).blocks[0]
    assert b0["recompute"] and b0["one_pass"]
    b0 = plan.plan_train(defs, dc._convs(defs), 2, 416, 416, conv0_one_pass=False).blocks[0]
    assert b0["recompute"] and not b0["one_pass"]
    assert not plan.plan_train(defs, dc._convs(defs), 2, 416, 416, conv0_recompute=False).blocks[0]["recompute"]
    src = open(plan.__file__).read()
    assert "import torch" not in src and "environ" not in src
