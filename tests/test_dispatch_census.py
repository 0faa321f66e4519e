"""CPU tier: the dispatch census (tests/dispatch_census.py) runs without a GPU (the library's kernel-choice calls are dry runs;
its CU count falls back to 256, the MI355X's), is deterministic, gives every edge class a representative, and names at 608^2 / bs 64
the kernels test_train_engine_gpu.py asserts of the training engine at that size."""
import ctypes as C

from tests import dispatch_census as dc


def _key(r):
    t = r["desc"]
    return "k%d s%d %d->%d @%d" % (t[5], t[6], t[3], t[4], dc._out_hw(t)[0])


def test_census_runs_is_deterministic_and_every_class_has_a_representative():
    refused = []
    a = dc.census(cus=256, refused=refused)
    b = dc.census(cus=256)
    assert list(a) == list(b)
    assert all(a[k]["count"] == b[k]["count"] and a[k]["rep"]["point"] == b[k]["rep"]["point"] for k in a)
    forms = set(k[0] for k in a)
    assert forms == {"eval", "pair", "head", "train", "dgrad", "wgrad"}, forms
    for key, e in a.items():
        r = e["rep"]
        assert e["count"] >= 1 and r["code"] >= 0, key
        assert dc.edge_class(r, 256) == key
    # yolov3-tiny with one class has 252-channel heads: the engine refuses it (channel counts must be multiples of 8)
    assert refused and all(p[0] == "tiny" and p[1] == 1 for p, _ in refused)
    print("\n%d edge classes" % len(a))


def test_census_names_the_bs64_kernels_the_engine_test_asserts():
    defs = dc.config_defs("darknet53", 1, 608, 608)
    recs = dc.train_blocks(defs, 608, 608, 64)
    fwd = {_key(r): dc.ops.kernel_name_of(r["code"], r["desc"][5], r["desc"][6], r["desc"][3]) for r in recs if r["form"] == "train"}
    dgr = {_key(r): dc.ops.kernel_name_of(r["code"], r["desc"][5], 1, r["desc"][4]) for r in recs if r["form"] == "dgrad"}
    assert fwd["k3 s1 128->256 @76"] == 'conv_mq<k3,128x256>' and fwd["k3 s1 256->512 @38"] == 'conv_mq<k3,128x256>'
    assert dgr["k3 s1 256->512 @38"] == 'conv_mq<k3,128x256>'
    assert fwd["k3 s1 64->128 @152"] == 'conv3x3_c64_halo' and fwd["k3 s2 64->128 @152"].startswith('conv_igemm<k3,128x128'), fwd
    assert dgr["k3 s1 128->256 @76"] == 'conv_igemm<k3,128x128>', dgr
    assert sum(1 for r in recs if r["form"] == "dgrad" and r["bnred"]) >= 40
    # 75 conv blocks; every one but layer 0 (one-pass backward) has a weight gradient and a data gradient
    assert sum(r["form"] == "train" for r in recs) == 75
    assert sum(r["form"] == "dgrad" for r in recs) == 74 and sum(r["form"] == "wgrad" for r in recs) == 74


def test_census_examples_of_the_issue():
    """the dry runs quoted when the census was asked for: bs 16 3x3 128->256 @76 (forward conv_mq, data gradient on the 128 x 128 tile,
    weight gradient on the wide tile), bs 1 3x3 512->1024 @10 (conv_mq with fewer tiles than workgroups), the nc = 2 head's weight
    gradient on the square 128 tile (not the 256-row one the 504-channel heads take)"""
    recs = dc.train_blocks(dc.config_defs("darknet53", 1, 608, 608), 608, 608, 16)
    by = {(r["form"], _key(r)): r for r in recs}
    assert dc.ops.kernel_name_of(by[("train", "k3 s1 128->256 @76")]["code"], 3, 1, 128) == 'conv_mq<k3,128x256>'
    assert by[("dgrad", "k3 s1 128->256 @76")]["code"] == 17
    assert by[("wgrad", "k3 s1 128->256 @76")]["code"] == 256
    recs = dc.train_blocks(dc.config_defs("darknet53", 1, 320, 320), 320, 320, 1)
    r = [r for r in recs if r["form"] == "train" and _key(r) == "k3 s1 512->1024 @10"][0]
    assert r["code"] == 3 and dc.edge_bits(r, 256)["underfull"]
    recs = dc.train_blocks(dc.config_defs("darknet53", 2, 608, 608), 608, 608, 16)
    heads = [r for r in recs if r["form"] == "wgrad" and r["desc"][4] == 576]
    assert len(heads) == 3 and all(r["code"] == 128 for r in heads)
    recs = dc.train_blocks(dc.config_defs("darknet53", 1, 608, 608), 608, 608, 16)
    assert all(r["code"] == 256 for r in recs if r["form"] == "wgrad" and r["desc"][4] == 504)
    L = dc._L()
    d = dc.mk_desc(heads[0]["desc"])
    assert L.ryolo_conv_wgrad_kernel_choice(C.byref(d)) == 128


def test_dry_run_queries_answer_the_same_from_two_threads():
    """The dry-run queries carry their launch context as an argument, so no state survives a call: two threads asking the forward-with-
    statistics, data-gradient, data-gradient-with-reduce and reduce-rows questions of the bs-64 training blocks at once, in opposite
    order, get the serial answers.  The blocks reach every reduce plan of the shipped library: conv_pw.hip (mode 1), the persistent 2x2
    tile (mode 2) and the one-tile-per-workgroup tiles (mode 3)."""
    import threading
    L = dc._L()
    recs = dc.train_blocks(dc.config_defs("darknet53", 1, 608, 608), 608, 608, 64)
    descs = {r["desc"]: r["stats"] for r in recs if r["form"] == "train"}
    queries = []
    for t, stats in descs.items():
        queries += [("fwd", t, 1 if stats else 0), ("dgrad", t, 0), ("dgrad", t, 1), ("rows", t, 0)]
    assert len(queries) >= 48

    def ask(q):
        what, t, flag = q
        d = dc.mk_desc(t)
        if what == "fwd":
            return L.ryolo_conv_kernel_choice(C.byref(d), 0, flag)
        if what == "dgrad":
            return L.ryolo_conv_dgrad_kernel_choice(C.byref(d), flag)
        return L.ryolo_conv2d_dgrad_bnreduce_rows(C.byref(d))

    serial = [ask(q) for q in queries]
    fused = set(a for q, a in zip(queries, serial) if q[0] == "dgrad" and q[2] == 1)
    # include/ryolo.h: RYOLO_CONV_KERNEL_PW = 6, RYOLO_CONV_KERNEL_IGEMM = 16 + tile code (7: the 2x2 tile, 1 / 2: 128 x 128 / 256 x 64)
    assert 6 in fused and 16 + 7 in fused and (16 + 1 in fused or 16 + 2 in fused), fused       # modes 1, 2, 3
    assert any(a > 0 for q, a in zip(queries, serial) if q[0] == "rows")

    PASSES = 50
    got = {}
    start = threading.Barrier(2)

    def worker(name, order):
        start.wait()
        got[name] = [[ask(queries[i]) for i in order] for _ in range(PASSES)]

    n = len(queries)
    threads = [threading.Thread(target=worker, args=("up", list(range(n)))),
               threading.Thread(target=worker, args=("down", list(range(n - 1, -1, -1))))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert got["up"] == [serial] * PASSES
    assert got["down"] == [serial[::-1]] * PASSES


def test_wgrad_host_decisions_match_the_golden():
    """Kernel code, workspace bytes and reduce job of every weight gradient of the census's input space (and of the bs-64 608^2 blocks
    under the tile bits 0x1000 / 0x2000 / 0x6000 / a forced split count) are the ones the library gave before its host code was rewritten
    around one plan: tests/golden/wgrad_plan.json holds one hash per (config, classes, H, W) group, generated from the parent commit's
    library by tests/golden/gen_wgrad_plan_golden.py."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan.json")) as fh:
        want = json.load(fh)["groups"]
    got = dc.wgrad_plan_hashes()
    assert sorted(got) == sorted(want)
    assert len(want) == 3 * len(dc.SIZES)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, "weight-gradient host decisions changed in %s" % differ


def test_conv_host_decisions_match_the_golden():
    """The kernel every forward convolution and data gradient takes (with and without residual, statistics and the folded BatchNorm
    reduce), the reduce's rows and the fused-op answers -- over the census's input space and, for a base set of plans, under every forced
    tile, tile bit, tuning switch and size guard -- are the ones the library gave before its dispatch was rewritten around one plan:
    tests/golden/conv_plan.json holds one hash per group, generated from the parent commit's library by
    tests/golden/gen_conv_plan_golden.py."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")) as fh:
        want = json.load(fh)["groups"]
    got = dc.conv_plan_hashes()
    assert sorted(got) == sorted(want)
    n_tune = sum(len(v) for _, v in dc.CONV_PLAN_TUNES)
    assert len(want) == len(dc.CONFIGS) * len(dc.SIZES) + len(dc.CONV_PLAN_PICKS) + len(dc.CONV_PLAN_BITS) + n_tune + 5
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, "convolution host decisions changed in %s" % differ


def test_data_gradient_refuses_more_pixels_than_a_launch_indexes():
    """The rows the golden records without data-gradient fields: an input gradient of more than 2^31 - 512 pixels.  The forward refuses
    such an output (conv_shape); the data gradient builds its launches through the same shape code and refuses too -- no kernel, no rows."""
    L = dc._L()
    groups = dc.conv_plan_groups(configs=(), sizes=(), batches=())
    rows = [r for g in groups.values() for r in g if r[0] not in ("pair", "head")]
    n = len(dc.DESC_FIELDS)
    big = [tuple(r[:n]) for r in rows if dc.dgrad_pixels(r) > dc.PIXELS_MAX]
    # every descriptor of guard/pixels is one (its forward output alone has too many pixels), stride-2 and 1x1 layers among them
    assert groups["guard/pixels"] and all(tuple(r[:n]) in big for r in groups["guard/pixels"])
    assert any(t[6] == 2 for t in big) and any(t[5] == 1 for t in big)
    for t in big:
        d = dc.mk_desc(t)
        got = (L.ryolo_conv_dgrad_kernel_choice(C.byref(d), 0), L.ryolo_conv_dgrad_kernel_choice(C.byref(d), 1), L.ryolo_conv2d_dgrad_bnreduce_rows(C.byref(d)))
        assert got == (-1, -1, 0), (t, got)


def test_wgrad_queries_answer_the_same_from_two_threads():
    """The weight gradient's queries compute one plan per call and keep nothing between calls: two threads asking the kernel choice, the
    workspace size and the reduce job of the bs-64 training blocks at once, in opposite order, get the serial answers."""
    import threading
    L = dc._L()
    recs = dc.train_blocks(dc.config_defs("darknet53", 1, 608, 608), 608, 608, 64)
    blocks = sorted(set((r["desc"], r["cin_real"]) for r in recs if r["form"] == "wgrad"))
    queries = [(what, t, c) for t, c in blocks for what in ("choice", "ws", "job")]
    assert len(queries) >= 48

    def ask(q):
        what, t, c = q
        d = dc.mk_desc(t)
        if what == "choice":
            return L.ryolo_conv_wgrad_kernel_choice(C.byref(d))
        if what == "ws":
            return L.ryolo_conv_wgrad_workspace_bytes(C.byref(d))
        return dc.wgrad_plan_record(t, c)[2:]

    serial = [ask(q) for q in queries]
    codes = set(a for q, a in zip(queries, serial) if q[0] == "choice")
    assert {256, 258, 259, 260}.issubset(codes) and any(a > dc.WGRAD_TAPS for a in codes), codes
    assert all(a > 0 for q, a in zip(queries, serial) if q[0] == "ws")
    assert all(a[-1] > 0 for q, a in zip(queries, serial) if q[0] == "job")         # block_end: the job was filled

    PASSES = 50
    got = {}
    start = threading.Barrier(2)

    def worker(name, order):
        start.wait()
        got[name] = [[ask(queries[i]) for i in order] for _ in range(PASSES)]

    n = len(queries)
    threads = [threading.Thread(target=worker, args=("up", list(range(n)))),
               threading.Thread(target=worker, args=("down", list(range(n - 1, -1, -1))))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert got["up"] == [serial] * PASSES
    assert got["down"] == [serial[::-1]] * PASSES
