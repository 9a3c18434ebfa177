"""CPU checks of what the four evaluation tools share (lav_amd.train.eval_common): the one layout class against the tables of the
three classes it replaced, written down from them; the tools' command lines against the tables of the parsers they had; the checkpoint
rule."""
import numpy as np
import pytest

from lav_amd import ops
from lav_amd.train import eval_common as X
from lav_amd.train import evaluate as E
from lav_amd.train import evaluate_bev as B
from lav_amd.train import evaluate_camera as C


# ------------------------------------------------------------------------------------------------------------ layouts
def _frame_table(nbins):
    return [("frames", 0, 1, ()), ("seg", 1, 10, (3, 3)), ("n_gt", 10, 12, (2,)), ("det", 12, 16, (2, 2)), ("plan", 16, 34, (6, 3)),
            ("plan_nonfinite", 34, 35, ()), ("oth_matched", 35, 36, ()), ("oth_unmatched", 36, 37, ()), ("oth_nonfinite", 37, 38, ()),
            ("oth_min", 38, 39, ()), ("oth_top", 39, 40, ()), ("oth_top_final", 40, 41, ()), ("hist", 41, 41 + 4 * nbins, (2, 2, nbins))]


def _map_table(name, at):
    return [(f"{name}.images", at, at + 1, ()), (f"{name}.pixels", at + 1, at + 2, ()), (f"{name}.ignored", at + 2, at + 3, ()),
            (f"{name}.nonfinite", at + 3, at + 4, ()), (f"{name}.conf", at + 4, at + 68, (8, 8))]


def _score_table(at, nbins):
    return [("scores.samples", at, at + 1, ()), ("scores.nonfinite", at + 1, at + 2, ()), ("scores.at", at + 2, at + 6, (2, 2)),
            ("scores.hist", at + 6, at + 6 + 2 * nbins, (2, nbins))]


# (layout, the library's or the header's word count, the parent commit's table of (name, start, stop, shape))
LAYOUTS = {
    "ACC": (E.ACC, lambda: ops.eval_acc_words(256), _frame_table(256)),
    "Layout(1)": (E.Layout(1), lambda: ops.eval_acc_words(1), _frame_table(1)),
    "Layout(1024)": (E.Layout(1024), lambda: ops.eval_acc_words(1024), _frame_table(1024)),
    "PlanLayout(1)": (B.PlanLayout(1), lambda: ops.eval_plans_words(1), [
        ("frames", 0, 1, ()), ("bad_cmd", 1, 2, ()), ("plan", 2, 74, (2, 2, 6, 3)), ("plan_nonfinite", 74, 76, (2,)), ("cmd_conf", 76, 112, (6, 6)),
        ("others", 112, 113, ()), ("oth_nonfinite", 113, 114, ()), ("oth", 114, 118, (4,)), ("oth_min_mode", 118, 124, (6,)),
        ("oth_top_mode", 124, 130, (6,)), ("oth_top_is_min", 130, 131, ())]),
    "PlanLayout(8)": (B.PlanLayout(8), lambda: ops.eval_plans_words(8), [
        ("frames", 0, 1, ()), ("bad_cmd", 1, 2, ()), ("plan", 2, 326, (2, 9, 6, 3)), ("plan_nonfinite", 326, 335, (9,)), ("cmd_conf", 335, 371, (6, 6)),
        ("others", 371, 372, ()), ("oth_nonfinite", 372, 373, ()), ("oth", 373, 377, (4,)), ("oth_min_mode", 377, 383, (6,)),
        ("oth_top_mode", 383, 389, (6,)), ("oth_top_is_min", 389, 390, ())]),
    "SEG": (C.SEG, lambda: 68, _map_table("seg", 0)),
    "BRA": (C.BRA, lambda: 68 + 68 + 6 + 2 * 256, _map_table("wide", 0) + _map_table("tele", 68) + _score_table(136, 256)),
    "ab10": (C.CameraLayout(("a", "b"), nbins=10), lambda: 68 + 68 + 6 + 2 * 10, _map_table("a", 0) + _map_table("b", 68) + _score_table(136, 10)),
}


def table_of(lay):
    """(name, start, stop, shape) of every field, read through the layout's views of an accumulator that holds its own indices."""
    index = np.arange(len(lay), dtype=np.int64)
    if not hasattr(lay, "maps"):
        views = {name: lay.view(index, name) for name in lay.fields}
    else:
        views = {f"{section}.{name}": v for section in lay.sections for name, v in lay.fields(index, section).items()}
    out = []
    for name, v in views.items():
        flat = v.reshape(-1)
        assert np.array_equal(flat, np.arange(flat[0], flat[0] + flat.size)), name       # contiguous, in order
        out.append((name, int(flat[0]), int(flat[-1]) + 1, v.shape))
    return out


@pytest.mark.parametrize("which", list(LAYOUTS))
def test_layout_is_the_parents_table_tiles_its_words_and_round_trips(which):
    lay, words, want = LAYOUTS[which]
    assert isinstance(lay, X.AccLayout)
    got = table_of(lay)
    assert got == want
    assert len(lay) == lay.words == words() == len(lay.zeros()) and lay.zeros().dtype == np.int64
    assert got[0][1] == 0 and got[-1][2] == len(lay) and all(a[2] == b[1] for a, b in zip(got, got[1:]))      # no gap, no overlap
    acc = (1 << 40) + np.random.default_rng(3).integers(-(1 << 20), 1 << 20, len(lay))
    named = lay.named(acc)
    np.testing.assert_array_equal(lay.unnamed(named), acc)
    if hasattr(lay, "maps"):
        assert list(named) == list(lay.sections) and [lay.kind(s) for s in lay.sections] == ["seg"] * len(lay.maps) + ["scores"] * (lay.nbins is not None)
    else:
        assert list(named) == [row[0] for row in want] and type(lay).of(acc).words == len(lay)


# ------------------------------------------------------------------------------------------------------------ command lines
_SHARED = {"--config-path": (None, None), "--data-dir": (None, None), "--num-workers": (4, None), "--seed": (2021, None),
           "--synthetic": (False, None), "--out": (None, None)}
_THREE = ("f16x3", "bf16x6", "f32", "all")
FLAGS = {       # option string -> (default, choices), from the parent commit's parsers
    "eval_full_v2": (E.TOOL, dict(_SHARED, **{"--lidar": (None, None), "--uniplanner": (None, None), "--bev": (None, None), "--precision": (None, _THREE),
                                               "--max-frames": (None, None), "--batch-size": (8, None), "--frames": (8, None),
                                               "--max-points": (None, None), "--match-radius": (2.0, None)})),
    "eval_seg": (C._WHAT["seg"], dict(_SHARED, **{"--seg": (None, None), "--precision": (None, ("f16x3", "bf16x6", "all")), "--max-images": (None, None),
                                                   "--batch-size": (24, None), "--frames": (6, None)})),
    "eval_bra_v2": (C._WHAT["bra"], dict(_SHARED, **{"--bra": (None, None), "--precision": (None, _THREE), "--max-frames": (None, None),
                                                      "--batch-size": (8, None), "--frames": (6, None)})),
    "eval_bev_v2": (B.TOOL, dict(_SHARED, **{"--bev": (None, None), "--precision": (None, _THREE), "--others": ("ahead", ("ahead", "all")),
                                              "--max-frames": (None, None), "--batch-size": (8, None), "--frames": (8, None)})),
}


@pytest.mark.parametrize("name", list(FLAGS))
def test_command_line_has_the_flags_defaults_and_choices_it_had(name):
    tool, want = FLAGS[name]
    assert tool["name"] == name
    got = {}
    for action in X.parser(tool)._actions:
        if action.dest != "help":
            assert len(action.option_strings) == 1
            got[action.option_strings[0]] = (action.default, None if action.choices is None else tuple(action.choices))
    assert got == want


# ------------------------------------------------------------------------------------------------------------ the checkpoint rule
def test_config_checkpoint(tmp_path):
    cfg = tmp_path / "config.yaml"
    rule = lambda given=None, synthetic=False: X.config_checkpoint(str(cfg), "seg_model_dir", "seg", given, synthetic, "for seeded weights")
    cfg.write_text(f"data_dir: {tmp_path}\n")                                    # the key absent
    with pytest.raises(SystemExit) as e:
        rule()
    assert "seg_model_dir" in str(e.value.code) and "--seg" in str(e.value.code) and str(cfg) in str(e.value.code)
    cfg.write_text("seg_model_dir: weights/seg_9.th\n")                          # the file absent
    with pytest.raises(SystemExit) as e:
        rule()
    assert "seg_model_dir: weights/seg_9.th" in str(e.value.code) and "--seg PATH" in str(e.value.code) and "for seeded weights" in str(e.value.code)
    (tmp_path / "weights").mkdir()
    (tmp_path / "weights" / "seg_9.th").write_bytes(b"")                         # a relative path: beside the config
    assert rule() == str(tmp_path / "weights" / "seg_9.th")
    assert rule(synthetic=True) is None                                          # --synthetic without the flag: seeded weights
    assert rule(given=str(tmp_path / "weights" / "seg_9.th"), synthetic=True) == str(tmp_path / "weights" / "seg_9.th")
    for synthetic in (False, True):                                              # a named file that is not there: an error even then
        with pytest.raises(SystemExit) as e:
            rule(given=str(tmp_path / "absent.th"), synthetic=synthetic)
        assert "absent.th" in str(e.value.code) and "seg_model_dir" in str(e.value.code) and "--seg" in str(e.value.code)
