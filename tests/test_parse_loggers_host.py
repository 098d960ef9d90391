"""evaluation.make_parse_logger / make_parse_score_logger on the host: a stub model replays fixed CPU tensors, and the printed line, the
returned dict (key order included) and the JSON record are compared with literals for every combination of the extras of a parse.

How EXPECTED was produced: this module's `run_case` was run for every entry of CASES against evaluation.py as of the commit BEFORE
the parse extras were gathered into evaluation._ParseExtras (commit 2315a72, "Optimal (Hungarian) track association and the IDF1
identity metric"), and the three results per logger were written out with repr().  The loggers must keep reproducing them byte for
byte; a figure that moves is a change of behaviour, not a reason to regenerate the table."""
import io
import itertools
import json

import numpy as np
import pytest
import torch

from attend_infer_repeat_amd import evaluation

B, T, G = 4, 3, 2
NAN, INF = float("nan"), float("inf")


def _batch(i, kw, nonfinite):
    """the parse of batch i (0 or 1) that `air.parse(**kw)` leaves: the tensors the loggers read"""
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    out = {"num_objects": torch.tensor([[1, 2, 0, 3], [2, 2, 1, 0]][i], dtype=i32),
           "count_prob": torch.tensor([[0.5, 0.25, 1.0, 0.125], [0.75, 0.5, 0.25, 0.0625]][i], dtype=f32)}
    if "particles" in kw:
        out["best_particle"] = torch.tensor([[0, 3, 1, 0], [2, 0, 0, 0]][i], dtype=i32)
        out["ess"] = torch.tensor([[1.5, 2.25, 4.0, 1.0], [3.5, 1.125, 2.0, 2.5]][i], dtype=f32)
    refined = {"objective": torch.tensor([[-10.5, -20.25, -5.0, -31.0], [-12.0, -8.5, -9.75, -40.0]][i], dtype=f64),
               "objective_start": torch.tensor([[-11.0, -20.25, -7.5, -33.0], [-12.5, -9.0, -9.75, -44.0]][i], dtype=f32)}
    if nonfinite:
        refined["objective"][1] = [NAN, INF][i]
        refined["objective_start"][3] = -INF
    if "refine" in kw:
        out.update(refined, best_iter=torch.tensor([[2, 0, 1, 4], [1, 3, 0, 2]][i], dtype=i32))
    if "prune" in kw or "propose" in kw:
        if "refine" in kw:
            out["refine_objective"], out["refine_objective_start"] = out["objective"], out["objective_start"]
        out["objective"] = torch.tensor([[-9.5, -19.0, -5.0, -30.5], [-11.25, -8.5, -9.0, -39.0]][i], dtype=f64)
        out["objective_start"] = torch.tensor([[-10.5, -20.25, -5.0, -31.0], [-12.0, -8.5, -9.75, -40.0]][i], dtype=f32)
        if nonfinite:
            out["objective"][0] = -INF
        out["num_objects_start"] = torch.tensor([[2, 2, 0, 2], [2, 3, 0, 0]][i], dtype=i32)
        out["best_mask"] = torch.tensor([[0b010, 0b011, 0b000, 0b111], [0b011, 0b101, 0b100, 0b000]][i], dtype=i32)
        out["kept_step"] = torch.zeros(T, B, dtype=i32)
    if "propose" in kw:
        out["objects_proposed_kept"] = torch.tensor([[0, 1, 0, 2], [1, 0, 1, 0]][i], dtype=i32)
    return out


class Scorer:
    thresholds_host = (0.5, 0.75)

    def __init__(self, log):
        self.log = log

    def reset(self):
        self.log.append("reset")

    def summary(self):
        return {"images": 2 * B, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125,
                "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625}


class Air:
    """parse / parse_scorer / score_parse of AIRonMNIST, replaying `_batch` in turn"""

    def __init__(self, nonfinite=False):
        self.obs, self.log, self.nonfinite, self.served = torch.zeros(B, 5, 5), [], nonfinite, 0

    def parse(self, obs, **kw):
        self.log.append(("parse", kw))
        self.parsed = _batch(self.served % 2, kw, self.nonfinite)
        self.served += 1
        return self.parsed

    def parse_scorer(self, max_gt_objects, **kw):
        self.log.append(("parse_scorer", max_gt_objects, kw))
        return Scorer(self.log)

    def score_parse(self, obs, gt_instances, gt_boxes, **kw):
        assert tuple(obs.shape) == (B, 5, 5) and tuple(gt_boxes.shape) == (B, G, 4)
        self.parse(obs, **kw)
        self.log[-1] = ("score_parse", kw)


def run_case(particles, refine, subset, nonfinite, capsys):
    """both loggers for one combination: {logger name: (printed line, returned dict, JSON line)} and the keyword dict every call got"""
    kw = dict(particles=particles, select="weight", refine=refine, refine_lr=None if refine is None else (0.01, 0.001), **subset)
    nums = torch.tensor([[[1], [1], [0], [1]], [[1], [1], [0], [1]], [[0], [0], [0], [1]]])          # [T, B, 1]: counts 2, 2, 0, 3
    data = dict(imgs=np.zeros((2 * B + 1, 5, 5), np.uint8), instances=np.zeros((2 * B + 1, 5, 5), np.int8),
                boxes=np.zeros((2 * B + 1, G, 4), np.float32))
    got, calls = {}, []
    for name, make in (("parse", lambda air, w: evaluation.make_parse_logger(air, lambda: (air.obs, nums), 2, "val", w, False, **kw)),
                       ("score", lambda air, w: evaluation.make_parse_score_logger(air, data, 5, "val", w, (0.5, 0.75), False, **kw))):
        air, writer = Air(nonfinite), io.StringIO()
        capsys.readouterr()
        acc = make(air, writer)(itr=7)
        got[name] = (capsys.readouterr().out, acc, writer.getvalue())
        calls += [e[-1] for e in air.log if isinstance(e, tuple)]
    return got, calls


SUBSETS = {"none": {}, "prune": dict(prune="all"), "propose": dict(propose=(1, 2))}
CASES = [(p, r, s, False) for p, r, s in itertools.product((None, 3), (None, 2), SUBSETS)] + [(None, 2, "prune", True),
                                                                                               (3, 2, "propose", True)]


@pytest.mark.parametrize("particles,refine,subset,nonfinite", CASES)
def test_the_parse_loggers_reproduce_the_recorded_lines(particles, refine, subset, nonfinite, capsys):
    got, calls = run_case(particles, refine, SUBSETS[subset], nonfinite, capsys)
    want_kw = {}
    if particles is not None:
        want_kw.update(particles=3, select="weight")
    if refine is not None:
        want_kw.update(refine=2, refine_lr=(0.01, 0.001))
    if subset != "none":
        want_kw.update({"prune": dict(prune="all"), "propose": dict(propose=[1, 2])}[subset])
    assert len(calls) == 2 + 1 + 2                                 # two parses; the scorer and two scored parses
    for kw in calls:                                               # what air.parse / parse_scorer / score_parse were given
        kw = {k: v for k, v in kw.items() if k != "thresholds"}
        assert kw == want_kw and list(kw) == list(want_kw)
    for name in ("parse", "score"):
        line, acc, record = got[name]
        want_line, want_acc, want_record = EXPECTED[(particles, refine, subset, nonfinite)][name]
        assert line == want_line
        assert acc == want_acc and list(acc) == list(want_acc)
        assert record == want_record and list(json.loads(record)) == list(json.loads(want_record))


def test_a_non_finite_gain_counts_as_zero(capsys):
    """images 1 and 3 of the refiner and image 0 of the pruner have a NaN or infinite gain: the means are those of the other images
    over ALL images"""
    got, _ = run_case(None, 2, SUBSETS["prune"], True, capsys)
    acc = got["parse"][1]
    assert acc["objective_gain"] == (0.5 + 2.5 + 0.5) / 8 and acc["prune_objective_gain"] == (1.25 + 0.5 + 0.75 + 1.0) / 8
    assert got["score"][1]["objective_gain"] == acc["objective_gain"]


EXPECTED = {
    (None, None, 'none', False): {
        'parse': ('Step 7, Data val parse map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375},
                  '{"step": 7, "data": "val_parse", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375}\n'),
        'score': ('Step 7, Data val parse score count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625}\n'),
    },
    (None, None, 'prune', False): {
        'parse': ('Step 7, Data val parse+prune(all) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "prune": "all", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score+prune(all) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "prune": "all", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "objective_gain": 0.65625}\n'),
    },
    (None, None, 'propose', False): {
        'parse': ('Step 7, Data val parse+propose([1, 2]) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, objects_added_from_residual = 0.6250, count_changed = 0.5000, objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "propose": [1, 2], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "objects_added_from_residual": 0.625, "count_changed": 0.5, "objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score+propose([1, 2]) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, objects_added_from_residual = 0.6250, count_changed = 0.5000, objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "propose": [1, 2], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "objects_added_from_residual": 0.625, "count_changed": 0.5, "objective_gain": 0.65625}\n'),
    },
    (None, 2, 'none', False): {
        'parse': ('Step 7, Data val parse+refine(2) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, objective_gain = 1.2500, refine_moved = 0.7500\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'objective_gain': 1.25, 'refine_moved': 0.75},
                  '{"step": 7, "data": "val_parse", "refine": 2, "refine_lr": [0.01, 0.001], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "objective_gain": 1.25, "refine_moved": 0.75}\n'),
        'score': ('Step 7, Data val parse score+refine(2) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, objective_gain = 1.2500, refine_moved = 0.7500\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'objective_gain': 1.25, 'refine_moved': 0.75},
                  '{"step": 7, "data": "val_parse_score", "refine": 2, "refine_lr": [0.01, 0.001], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "objective_gain": 1.25, "refine_moved": 0.75}\n'),
    },
    (None, 2, 'prune', False): {
        'parse': ('Step 7, Data val parse+refine(2)+prune(all) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, objective_gain = 1.2500, refine_moved = 0.7500, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, prune_objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'objective_gain': 1.25, 'refine_moved': 0.75, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'prune_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "refine": 2, "refine_lr": [0.01, 0.001], "prune": "all", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "objective_gain": 1.25, "refine_moved": 0.75, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "prune_objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score+refine(2)+prune(all) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, objective_gain = 1.2500, refine_moved = 0.7500, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, prune_objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'objective_gain': 1.25, 'refine_moved': 0.75, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'prune_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "refine": 2, "refine_lr": [0.01, 0.001], "prune": "all", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "objective_gain": 1.25, "refine_moved": 0.75, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "prune_objective_gain": 0.65625}\n'),
    },
    (None, 2, 'propose', False): {
        'parse': ('Step 7, Data val parse+refine(2)+propose([1, 2]) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, objective_gain = 1.2500, refine_moved = 0.7500, objects_added_from_residual = 0.6250, count_changed = 0.5000, propose_objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'objective_gain': 1.25, 'refine_moved': 0.75, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'propose_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "refine": 2, "refine_lr": [0.01, 0.001], "propose": [1, 2], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "objective_gain": 1.25, "refine_moved": 0.75, "objects_added_from_residual": 0.625, "count_changed": 0.5, "propose_objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score+refine(2)+propose([1, 2]) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, objective_gain = 1.2500, refine_moved = 0.7500, objects_added_from_residual = 0.6250, count_changed = 0.5000, propose_objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'objective_gain': 1.25, 'refine_moved': 0.75, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'propose_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "refine": 2, "refine_lr": [0.01, 0.001], "propose": [1, 2], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "objective_gain": 1.25, "refine_moved": 0.75, "objects_added_from_residual": 0.625, "count_changed": 0.5, "propose_objective_gain": 0.65625}\n'),
    },
    (3, None, 'none', False): {
        'parse': ('Step 7, Data val parse(3, weight) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375}\n'),
        'score': ('Step 7, Data val parse score(3, weight) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375}\n'),
    },
    (3, None, 'prune', False): {
        'parse': ('Step 7, Data val parse(3, weight)+prune(all) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "prune": "all", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score(3, weight)+prune(all) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "prune": "all", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "objective_gain": 0.65625}\n'),
    },
    (3, None, 'propose', False): {
        'parse': ('Step 7, Data val parse(3, weight)+propose([1, 2]) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344, objects_added_from_residual = 0.6250, count_changed = 0.5000, objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "propose": [1, 2], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375, "objects_added_from_residual": 0.625, "count_changed": 0.5, "objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score(3, weight)+propose([1, 2]) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344, objects_added_from_residual = 0.6250, count_changed = 0.5000, objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "propose": [1, 2], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375, "objects_added_from_residual": 0.625, "count_changed": 0.5, "objective_gain": 0.65625}\n'),
    },
    (3, 2, 'none', False): {
        'parse': ('Step 7, Data val parse(3, weight)+refine(2) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 1.2500, refine_moved = 0.7500\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 1.25, 'refine_moved': 0.75},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 1.25, "refine_moved": 0.75}\n'),
        'score': ('Step 7, Data val parse score(3, weight)+refine(2) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 1.2500, refine_moved = 0.7500\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 1.25, 'refine_moved': 0.75},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 1.25, "refine_moved": 0.75}\n'),
    },
    (3, 2, 'prune', False): {
        'parse': ('Step 7, Data val parse(3, weight)+refine(2)+prune(all) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 1.2500, refine_moved = 0.7500, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, prune_objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 1.25, 'refine_moved': 0.75, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'prune_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "prune": "all", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 1.25, "refine_moved": 0.75, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "prune_objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score(3, weight)+refine(2)+prune(all) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 1.2500, refine_moved = 0.7500, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, prune_objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 1.25, 'refine_moved': 0.75, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'prune_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "prune": "all", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 1.25, "refine_moved": 0.75, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "prune_objective_gain": 0.65625}\n'),
    },
    (3, 2, 'propose', False): {
        'parse': ('Step 7, Data val parse(3, weight)+refine(2)+propose([1, 2]) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 1.2500, refine_moved = 0.7500, objects_added_from_residual = 0.6250, count_changed = 0.5000, propose_objective_gain = 0.6562\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 1.25, 'refine_moved': 0.75, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'propose_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "propose": [1, 2], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 1.25, "refine_moved": 0.75, "objects_added_from_residual": 0.625, "count_changed": 0.5, "propose_objective_gain": 0.65625}\n'),
        'score': ('Step 7, Data val parse score(3, weight)+refine(2)+propose([1, 2]) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 1.2500, refine_moved = 0.7500, objects_added_from_residual = 0.6250, count_changed = 0.5000, propose_objective_gain = 0.6562\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 1.25, 'refine_moved': 0.75, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'propose_objective_gain': 0.65625},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "propose": [1, 2], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 1.25, "refine_moved": 0.75, "objects_added_from_residual": 0.625, "count_changed": 0.5, "propose_objective_gain": 0.65625}\n'),
    },
    (None, 2, 'prune', True): {
        'parse': ('Step 7, Data val parse+refine(2)+prune(all) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, objective_gain = 0.4375, refine_moved = 0.7500, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, prune_objective_gain = 0.4375\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'objective_gain': 0.4375, 'refine_moved': 0.75, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'prune_objective_gain': 0.4375},
                  '{"step": 7, "data": "val_parse", "refine": 2, "refine_lr": [0.01, 0.001], "prune": "all", "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "objective_gain": 0.4375, "refine_moved": 0.75, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "prune_objective_gain": 0.4375}\n'),
        'score': ('Step 7, Data val parse score+refine(2)+prune(all) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, objective_gain = 0.4375, refine_moved = 0.7500, count_changed = 0.5000, objects_dropped = 0.2500, objects_added = 0.2500, prune_objective_gain = 0.4375\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'objective_gain': 0.4375, 'refine_moved': 0.75, 'count_changed': 0.5, 'objects_dropped': 0.25, 'objects_added': 0.25, 'prune_objective_gain': 0.4375},
                  '{"step": 7, "data": "val_parse_score", "refine": 2, "refine_lr": [0.01, 0.001], "prune": "all", "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "objective_gain": 0.4375, "refine_moved": 0.75, "count_changed": 0.5, "objects_dropped": 0.25, "objects_added": 0.25, "prune_objective_gain": 0.4375}\n'),
    },
    (3, 2, 'propose', True): {
        'parse': ('Step 7, Data val parse(3, weight)+refine(2)+propose([1, 2]) map_num_step_acc = 0.6250, count_prob = 0.4297, num_objects = 1.3750, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 0.4375, refine_moved = 0.7500, objects_added_from_residual = 0.6250, count_changed = 0.5000, propose_objective_gain = 0.4375\n',
                  {'map_num_step_acc': 0.625, 'count_prob': 0.4296875, 'num_objects': 1.375, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 0.4375, 'refine_moved': 0.75, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'propose_objective_gain': 0.4375},
                  '{"step": 7, "data": "val_parse", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "propose": [1, 2], "map_num_step_acc": 0.625, "count_prob": 0.4296875, "num_objects": 1.375, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 0.4375, "refine_moved": 0.75, "objects_added_from_residual": 0.625, "count_changed": 0.5, "propose_objective_gain": 0.4375}\n'),
        'score': ('Step 7, Data val parse score(3, weight)+refine(2)+propose([1, 2]) count_acc = 0.6250, map = 0.4375, ap@0.50 = 0.5000, fg_ari = 0.8125, mean_best_overlap = 0.7188, matched_box_iou = 0.6562, best_particle_moved = 0.3750, ess = 2.2344, objective_gain = 0.4375, refine_moved = 0.7500, objects_added_from_residual = 0.6250, count_changed = 0.5000, propose_objective_gain = 0.4375\n',
                  {'images': 8, 'count_acc': 0.625, 'map': 0.4375, 'ap@0.50': 0.5, 'ap@0.75': 0.375, 'fg_ari': 0.8125, 'mean_best_overlap': 0.71875, 'matched_box_iou': 0.65625, 'best_particle_moved': 0.375, 'ess': 2.234375, 'objective_gain': 0.4375, 'refine_moved': 0.75, 'objects_added_from_residual': 0.625, 'count_changed': 0.5, 'propose_objective_gain': 0.4375},
                  '{"step": 7, "data": "val_parse_score", "particles": 3, "select": "weight", "refine": 2, "refine_lr": [0.01, 0.001], "propose": [1, 2], "images": 8, "count_acc": 0.625, "map": 0.4375, "ap@0.50": 0.5, "ap@0.75": 0.375, "fg_ari": 0.8125, "mean_best_overlap": 0.71875, "matched_box_iou": 0.65625, "best_particle_moved": 0.375, "ess": 2.234375, "objective_gain": 0.4375, "refine_moved": 0.75, "objects_added_from_residual": 0.625, "count_changed": 0.5, "propose_objective_gain": 0.4375}\n'),
    },
}
