"""CPU tier: plan_train(..., trainable=...) -- the training plan of a partly frozen model (rotate-yolov3_amd/model/plan.py).

Darknet-53 at 64 x 64, batch 2.  What must need a gradient is computed HERE, by reachability over the cfg's own edges (conv input,
shortcut source, route sources, upsample input), not with the planner's helpers; the plan is then held against it: which backward
entries remain, what each conv entry launches (dgrad / wgrad), grd[i] is None exactly where no gradient is needed, every plan buffer
is referenced, every live gradient view has exactly one first writer among the entries that remain.

Pattern E of the issue names "block 43": layer 43 of this cfg is the shortcut that closes the residual unit 41-42-43 and has no
parameter of its own; the trainable weight is that of conv 42, the conv that computes layer 43's tensor (its shortcut is folded into it).

tests/golden/train_plan_d53_64.json is the plan of the commit before `trainable` existed, with the buffer ids renumbered in order of
first appearance (that plan also listed 21 gradient buffers that no view referenced; they are gone, the views are the same)."""
import json
import os

import pytest

from tests import dispatch_census as dc
from rotate_yolov3_amd.cfg import make_cfg
from rotate_yolov3_amd.model import plan
from rotate_yolov3_amd.utils.parse_config import parse_model_cfg_text

N, H, W = 2, 64, 64
HEADS = (81, 93, 105)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plan_d53_64.json")
VIEW_KEYS = ("xin", "xin_g", "y", "dy", "res", "res_g")
FLAG_KEYS = ("bnbwd", "dgrad", "wgrad")


def _defs():
    defs = parse_model_cfg_text(make_cfg.darknet53(W, H))
    assert defs[0]["type"] == "net"
    return defs[1:]


DEFS = _defs()
CONVS = dc._convs(DEFS)
ALL = {i: (True, True, True) for i in CONVS}


def _pattern(name):
    if name == "A":          # --transfer: the convs in front of the yolo layers, weight and bias
        return {i: (True, True, False) for i in HEADS}
    if name == "B":          # --prebias: their biases only
        return {i: (False, True, False) for i in HEADS}
    if name == "C":          # trunk frozen
        return {i: (i >= 75,) * 3 for i in CONVS}
    if name == "D":          # island: block 80's weight and BatchNorm are frozen, everything else trains
        return dict(list(ALL.items()) + [(80, (False, False, True))])
    if name == "E":          # one trainable weight deep in the trunk (see the module docstring)
        return {42: (True, False, False)}
    raise KeyError(name)


def _abs(i, l):
    return l if l > 0 else i + l


def _inputs(i):
    d = DEFS[i]
    if d["type"] == "route":
        return [_abs(i, int(v)) for v in d["layers"].split(",")]
    ins = [i - 1] if i > 0 else []
    if d["type"] == "shortcut":
        ins.append(_abs(i, int(d["from"])))
    return ins


def _needs(trainable):
    """layer -> its output needs a gradient: a trainable parameter lies in a layer it depends on"""
    memo = {}

    def need(i):
        if i not in memo:
            memo[i] = any(trainable.get(i, ())) or any(need(j) for j in _inputs(i))
        return memo[i]
    return [need(i) for i in range(len(DEFS))]


def _build(trainable):
    return plan.plan_train(DEFS, CONVS, N, H, W, yolos=dc._yolos(DEFS), trainable=trainable)


def _out_layer(tp, kind, i):
    """the layer whose tensor a forward entry computes: a conv with its shortcut folded in computes the shortcut's"""
    folded = kind == "conv" and i + 1 < len(DEFS) and DEFS[i + 1]["type"] == "shortcut" and not any(
        k == "add" and j == i + 1 for k, j, _ in tp.forward)
    return i + 1 if folded else i


def _grad_views(tp):
    live = set(v for v in tp.grd if v is not None)
    for kind, i, pl in tp.forward:
        if kind == "conv":
            live.update(v for v in (pl["xin_g"], pl["dy"], pl["res_g"]) if v is not None)
        elif kind == "add":
            live.update(v for v in pl[3:] if v is not None)
        elif kind == "up":
            live.update(v for v in pl[2:] if v is not None)
        else:
            live.update(v for v in pl[1:] if v is not None)
    return live


def _check_first_writers(tp):
    """replays the remaining backward entries: a FIRST writer writes channels nobody wrote, any other accumulates onto channels that are
    all written, every gradient an entry reads was written -- so each live gradient view has exactly one first writer.  Returns the
    views that were written."""
    w = {}

    def chans(v):
        return set(range(v.off, v.off + v.C))

    def write(v, first, who):
        if first:
            assert not (chans(v) & w.get(v.buf, set())), ("a second first writer", who, v)
            w.setdefault(v.buf, set()).update(chans(v))
        else:
            assert chans(v) <= w.get(v.buf, set()), ("accumulates onto an uninitialised gradient", who, v)

    recs = {(k, i): pl for k, i, pl in tp.forward}
    written = set()
    for kind, i, flags in tp.backward:
        pl = recs[(kind, i)]
        if kind == "yolo":
            write(pl[1], True, (kind, i))
            written.add(pl[1])
            continue
        dy = pl["dy"] if kind == "conv" else (pl[5] if kind == "add" else pl[3])
        assert dy is not None and chans(dy) <= w.get(dy.buf, set()), ("reads a gradient nobody wrote", kind, i, dy)
        if kind == "conv":
            outs = [(pl["res_g"] if not pl["res_alias"] else None, flags[0]), (pl["xin_g"] if pl["dgrad"] else None, flags[1])]
        elif kind == "add":
            outs = list(zip(pl[3:5], flags))
        else:
            outs = [(pl[2], flags)]
        for v, f in outs:
            assert (v is None) == (f is None), (kind, i, v, f)
            if v is not None:
                write(v, f, (kind, i))
                written.add(v)
    return written


def _check(tp, trainable):
    need = _needs(trainable)
    # the set of entries that run
    want = [(k, i) for k, i, _ in reversed(tp.forward) if need[_out_layer(tp, k, i)]]
    assert [(k, i) for k, i, _ in tp.backward] == want
    # what each conv entry launches
    for b in tp.blocks:
        i = b["layer"]
        assert b["bnbwd"] == need[i], i
        assert b["dgrad"] == (need[i] and i > 0 and need[i - 1]), i
        assert b["wgrad"] == bool(trainable.get(i, (False,))[0]), i
        assert (b["xin_g"] is not None) == b["dgrad"] and (b["dy"] is not None) == need[_out_layer(tp, "conv", i)], i
    # grd[i] is None exactly where no gradient is needed
    assert [g is not None for g in tp.grd] == need
    # every plan buffer is referenced by an activation view or a live gradient view
    live = _grad_views(tp)
    used = set(v.buf for v in tp.act if v is not None) | set(v.buf for v in live) | {tp.x.buf}
    assert used == set(range(len(tp.buffers))), sorted(set(range(len(tp.buffers))) - used)
    # each live gradient view has exactly one first writer among the remaining entries (a slice of a concat gradient is written with it)
    written = _check_first_writers(tp)
    for v in live:
        assert any(u.buf == v.buf and u.off <= v.off and v.off + v.C <= u.off + u.C for u in written), ("never written", v)
    return need


def _layers(tp, kind=None):
    return sorted(i for k, i, _ in tp.backward if kind is None or k == kind)


def test_transfer_runs_the_three_head_convs_and_nothing_else():
    tr = _pattern("A")
    tp = _build(tr)
    _check(tp, tr)
    assert _layers(tp, "conv") == list(HEADS) and _layers(tp, "yolo") == [82, 94, 106] and len(tp.backward) == 6
    by = {b["layer"]: b for b in tp.blocks}
    assert all(by[i]["wgrad"] and not by[i]["dgrad"] for i in HEADS)
    assert sum(g is not None for g in tp.grd) == 6          # the head convs' outputs and the yolo layers that alias them


def test_prebias_runs_the_head_entries_without_any_weight_gradient():
    tr = _pattern("B")
    tp = _build(tr)
    _check(tp, tr)
    assert _layers(tp, "conv") == list(HEADS)
    assert not any(b["wgrad"] or b["dgrad"] for b in tp.blocks) and all(b["bnbwd"] == (b["layer"] in HEADS) for b in tp.blocks)


def test_frozen_trunk_stops_the_backward_at_layer_75():
    tr = _pattern("C")
    tp = _build(tr)
    need = _check(tp, tr)
    assert min(_layers(tp)) == 75 and not any(need[:75]) and all(need[75:])
    by = {b["layer"]: b for b in tp.blocks}
    # 75 reads the trunk, 87 / 99 read concats of a head tensor and a trunk tensor (61, 36): the concat gradient exists, the trunk's slice not
    assert not by[75]["dgrad"] and by[87]["dgrad"] and by[99]["dgrad"] and tp.grd[61] is None and tp.grd[36] is None
    assert all(b["wgrad"] == (b["layer"] >= 75) for b in tp.blocks)


def test_a_frozen_island_still_passes_the_gradient_through():
    tr = _pattern("D")
    tp = _build(tr)
    need = _check(tp, tr)
    assert all(need)
    by = {b["layer"]: b for b in tp.blocks}
    assert by[80]["bnbwd"] and by[80]["dgrad"] and not by[80]["wgrad"]
    assert all(b["wgrad"] for b in tp.blocks if b["layer"] != 80)
    # the same entries, views and first-writer flags as with everything trainable; only block 80's wgrad flag differs
    full = _build(None)
    assert tp.backward == full.backward and tp.grd == full.grd and tp.buffers == full.buffers
    assert [dict(b, wgrad=True) for b in tp.blocks] == full.blocks


def test_one_trainable_weight_deep_in_the_trunk():
    tr = _pattern("E")
    tp = _build(tr)
    need = _check(tp, tr)
    assert need == [i >= 42 for i in range(len(DEFS))]        # all three heads depend on the unit, nothing below it does
    assert min(_layers(tp)) == 42 and set(_layers(tp, "yolo")) == {82, 94, 106}
    assert [b["layer"] for b in tp.blocks if b["wgrad"]] == [42]
    by = {b["layer"]: b for b in tp.blocks}
    assert by[42]["bnbwd"] and not by[42]["dgrad"] and by[42]["res_g"] is None and by[44]["dgrad"]
    assert tp.grd[36] is None and tp.grd[61] is not None and tp.grd[98] is not None


def _canon(tp):
    """the plan as JSON data with buffer ids renumbered in order of first appearance (x, act, grd, forward records)"""
    ids = {}

    def cv(v):
        return None if v is None else [ids.setdefault(v.buf, len(ids))] + [int(t) for t in v[1:]]

    out = dict(x=cv(tp.x), act=[cv(v) for v in tp.act], grd=[cv(v) for v in tp.grd], forward=[])
    for kind, i, pl in tp.forward:
        if kind == "conv":
            rec = {k: (cv(v) if k in VIEW_KEYS else v) for k, v in sorted(pl.items()) if k not in FLAG_KEYS}
        else:
            rec = [cv(v) for v in pl]
        out["forward"].append([kind, i, rec])
    out["backward"] = [[k, i, f] for k, i, f in tp.backward]
    out["shapes"] = [list(s) for s in tp.shapes]
    out["buffers"] = [list(tp.buffers[b]) for b in sorted(ids, key=ids.get)]
    return json.loads(json.dumps(out))


def test_everything_trainable_is_the_plan_of_before():
    none, full = _build(None), _build(ALL)
    assert none == full
    _check(none, ALL)
    assert [(k, i) for k, i, _ in none.backward] == [(k, i) for k, i, _ in reversed(none.forward)]
    assert all(b["bnbwd"] and b["wgrad"] and b["dgrad"] == (b["layer"] > 0) for b in none.blocks)
    with open(GOLDEN) as fh:        # (recorded without `yolos`, that is without the fused-head records)
        assert _canon(plan.plan_train(DEFS, CONVS, N, H, W)) == json.load(fh)
        assert _canon(plan.plan_train(DEFS, CONVS, N, H, W, trainable=ALL)) == _canon(plan.plan_train(DEFS, CONVS, N, H, W))


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_a_frozen_plan_keeps_the_views_and_flags_of_what_still_runs(name):
    """the entries that remain read and write the gradients they did (same shapes, same residual aliasing, same FIRST flags): the bits
    of a trainable gradient cannot depend on what is frozen"""
    tr = _pattern(name)
    tp, full = _build(tr), _build(None)
    fb = {(k, i): f for k, i, f in full.backward}
    fr = {(k, i): pl for k, i, pl in full.forward}
    shape = lambda v: None if v is None else tuple(v[1:])      # noqa: E731
    recs = {(k, i): pl for k, i, pl in tp.forward}
    for kind, i, flags in tp.backward:
        pl, old = recs[(kind, i)], fr[(kind, i)]
        if kind == "conv":
            assert shape(pl["dy"]) == shape(old["dy"]) and pl["res_alias"] == (old["res_alias"] and pl["res_g"] is not None)
            for k, (f, g) in enumerate(zip(flags, fb[(kind, i)])):
                assert f is None or f == g, (kind, i, k, flags, fb[(kind, i)])
        elif kind == "add":
            assert all(f is None or f == g for f, g in zip(flags, fb[(kind, i)]))
        elif kind == "up":
            assert flags is None or flags == fb[(kind, i)]


def test_the_records_are_named_and_a_conv_block_has_no_undeclared_state():
    """AddRec / UpRec / YoloRec are the plain tuples they replaced; a TrainEngine ConvBlock refuses a misspelt attribute"""
    from rotate_yolov3_amd.model.train_engine import ConvBlock
    # Darknet-53's shortcuts are all folded into their convs: a second shortcut behind its first unit is a stand-alone add
    small = DEFS[:5] + [{"type": "shortcut", "from": "-4", "activation": "linear"}]
    seen = set()
    for defs, tp in ((small, plan.plan_train(small, dc._convs(small), N, H, W)), (DEFS, _build(None))):
        for kind, i, pl in tp.forward:
            if kind == "add":
                a, b = i - 1, plan._abs(i, int(defs[i]["from"]))
                assert type(pl) is plan.AddRec and pl == (tp.act[a], tp.act[b], tp.act[i], tp.grd[a], tp.grd[b], tp.grd[i])
                assert (pl.a, pl.b, pl.y, pl.a_g, pl.b_g, pl.dy) == tuple(pl)
            elif kind == "up":
                assert type(pl) is plan.UpRec and pl == (tp.act[i - 1], tp.act[i], tp.grd[i - 1], tp.grd[i])
                assert (pl.x, pl.y, pl.x_g, pl.dy) == tuple(pl)
            elif kind == "yolo":
                assert type(pl) is plan.YoloRec and pl == (tp.act[i], tp.grd[i]) and (pl.head, pl.head_g) == tuple(pl)
            seen.add(kind)
    assert seen == {"conv", "add", "up", "yolo"}
    blk = ConvBlock.__new__(ConvBlock)
    blk.head_k = 1
    with pytest.raises(AttributeError):
        blk.head_kk = 1
    assert not hasattr(blk, "__dict__")
