"""CPU tier: train.py --transfer / --prebias -- the flags are real, the freeze rule and the lr / momentum scaling mirror the reference
(train.py:120-135), and `--prebias` runs end to end: one bias-only epoch, <wdir>/backbone.pt, then the normal run from it."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HYP_TEXT = ("giou: 0.1\ncls: 27.76\ncls_pw: 1.446\nobj: 20.35\nobj_pw: 3.941\niou_t: 0.3\nang_t: 3.1415926/12\n"
            "reg: 1.0\nfl_gamma: 0.5\ncontext_factor: 1.0\nlr0: 0.0001\nmultiplier:10\nwarm_epoch:1\nmomentum: 0.97\n"
            "weight_decay: 0.0004569\nepochs: 2\nbatch_size: 2\nsave_interval: 300\ntest_interval: 5\n")     # tests/test_train_entry.py's
HYP = {"lr0": 1e-3, "momentum": 0.9, "weight_decay": 5e-4, "multiplier": 10.0, "warm_epoch": 1, "context_factor": 1.0}


def test_transfer_and_prebias_are_no_longer_ignored_flags():
    import train
    from rotate_yolov3_amd.utils.cli import report_ignored
    for flag in ("--transfer", "--prebias"):
        parser, ignored, opt = train.parse_args([flag])
        assert getattr(opt, flag[2:]) is True
        assert report_ignored(parser, opt, ignored, out=lambda s: None) == []
    parser, ignored, opt = train.parse_args(["--rect"])          # (the list still works for what stays in it)
    assert report_ignored(parser, opt, ignored, out=lambda s: None) == ["rect"]


def _darknet53():
    from rotate_yolov3_amd.cfg import make_cfg
    from rotate_yolov3_amd.model.models import Darknet
    return Darknet(make_cfg.darknet53(64, 64), {"context_factor": 1.0})


def test_the_freeze_rule_selects_six_tensors_for_transfer_and_three_for_prebias():
    import train
    model = _darknet53()
    names = {p: k for k, p in model.named_parameters()}
    heads = [i - 1 for i in model.yolo_layers]
    assert heads == [81, 93, 105]
    for kw, want in ((dict(transfer=True), ["Conv2d.weight", "Conv2d.bias"]), (dict(prebias=True), ["Conv2d.bias"]),
                     (dict(transfer=True, prebias=True), ["Conv2d.bias"])):       # the reference tests prebias first
        opt = train.make_optimizer(model, HYP, fused=False)
        kept = train.freeze_for_transfer(model, opt, **kw)
        assert sorted(names[p] for p in kept) == sorted("module_list.%d.%s" % (i, w) for i in heads for w in want)
        assert [p for p in model.parameters() if p.requires_grad] == kept
        assert len(kept) == 3 * len(want)


def test_lr_and_momentum_of_every_group_and_the_schedule_base_are_scaled():
    import train
    for adam in (False, True):
        model = _darknet53()
        opt = train.make_optimizer(model, HYP, adam=adam, fused=False)
        before = [dict(g) for g in opt.param_groups]
        assert len(before) == 2
        train.freeze_for_transfer(model, opt, transfer=True)
        train.init_schedule(opt, HYP, train.TRANSFER_LR_SCALE)
        for g, b in zip(opt.param_groups, before):
            assert g["lr"] == b["lr"] * 100 and g["initial_lr"] == HYP["lr0"] * 100
            if adam:
                assert "momentum" not in g and g["betas"] == b["betas"]
            else:
                assert g["momentum"] == b["momentum"] * 0.9
        f = train.set_epoch_lr(opt, HYP, 1, 20)               # the end of the warm-up: lr0 x 100 x multiplier
        assert f == 10.0 and all(abs(g["lr"] - HYP["lr0"] * 100 * 10) < 1e-12 for g in opt.param_groups)
    # without the flags nothing is scaled
    opt = train.make_optimizer(_darknet53(), HYP, fused=False)
    train.init_schedule(opt, HYP)
    assert all(g["initial_lr"] == HYP["lr0"] and g["lr"] == HYP["lr0"] and g["momentum"] == HYP["momentum"] for g in opt.param_groups)


def test_print_model_biases_views_the_bias_by_the_heads_own_anchor_count():
    import train
    model = _darknet53()
    with torch.no_grad():
        for l in model.yolo_layers:
            b = model.module_list[l - 1][0].bias.view(model.module_list[l].na, -1)
            assert b.shape == (72, 7)
            b[:, :5] = 1.0
            b[:, 5] = -4.0
            b[:, 6:] = 2.0
    lines = []
    train.print_model_biases(model, out=lines.append)
    assert len(lines) == 4 and "Model Bias Summary" in lines[0]
    for s in lines[1:]:
        assert "regression:  1.00+/-0.00" in s and "objectness: -4.00+/-0.00" in s and "classification:  2.00+/-" in s, s


def test_train_py_prebias_end_to_end(tmp_path, monkeypatch, capsys):
    import train
    from tests.test_dp_gloo import CFG
    from rotate_yolov3_amd.model.models import Darknet
    from rotate_yolov3_amd.utils.parse_config import hyp_parse
    from rotate_yolov3_amd.utils.torch_utils import init_seeds
    cfg = tmp_path / "m.cfg"
    cfg.write_text(CFG)
    hyp = tmp_path / "hyp.py"
    hyp.write_text(HYP_TEXT)
    monkeypatch.chdir(tmp_path)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    wdir = tmp_path / "w"
    train.main(["--cfg", str(cfg), "--hyp", str(hyp), "--img-size", "64", "--synthetic", "4", "--device", "cpu", "--wdir", str(wdir),
                "--prebias"])
    out = capsys.readouterr().out
    # one prebias epoch (a bias summary instead of an evaluation), then the normal run of hyp's two epochs
    assert out.count("Model Bias Summary") == 1 and out.count("epochs completed") == 2 and "1 epochs completed" in out
    rows = (tmp_path / "results.txt").read_text().strip().split("\n")
    assert len(rows) == 3 and [r.split()[0] for r in rows] == ["0/0", "0/1", "1/1"]
    bb = torch.load(str(wdir / "backbone.pt"))
    assert set(bb) == {"epoch", "best_fitness", "training_results", "model", "optimizer"}
    assert bb["epoch"] == -1 and bb["optimizer"] is None and bb["training_results"] is None
    last = torch.load(str(wdir / "last.pt"))
    assert last["epoch"] == 1
    # after the prebias epoch only the head biases differ from the initial state dict, apart from the BatchNorm running statistics
    init_seeds()
    first = Darknet(str(cfg), hyp_parse(str(hyp)), arc="defaultpw")
    sd0 = first.state_dict()
    biases = set("module_list.%d.Conv2d.bias" % (l - 1) for l in first.yolo_layers)
    assert len(biases) == 2 and set(sd0) == set(bb["model"])
    changed = set(k for k, v in sd0.items() if not torch.equal(v, bb["model"][k]))
    stats = set(k for k in sd0 if k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    assert changed - stats == biases, sorted(changed - stats)
    assert stats <= changed                                       # frozen BatchNorm layers keep training-mode statistics
    # ... and the normal run that followed trained everything again
    later = set(k for k, v in sd0.items() if not torch.equal(v, last["model"][k]))
    assert later == set(sd0)
