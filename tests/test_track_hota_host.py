"""Host tests of the HOTA metric (attend_infer_repeat_amd/track.py: reference_hota, hota_summary): the closed forms, an independent
TrackEval-style evaluation (float scores, scipy's solver, alpha - eps), the thresholds at equality, the tie rule, the conventions of
the summary, the refusals, the entry's prototype, and planted defects of the reference that the closed forms catch."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from track_hota_cases import CRAFTED, hota_case, stack, trackeval_case

from attend_infer_repeat_amd import _lib, track

ROOT = Path(__file__).resolve().parents[1]
NA = 19
FIGURES = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")


def reference(case, **kw):
    return track.reference_hota(case["boxes"], case["n"], case["ids"], case["gt"], case["F"], case.get("n_ids"), **kw)


def summary(case):
    ref = reference(case)
    return track.hota_summary(ref["seq_hota_i"].sum(0), ref["seq_hota_f"].sum(0)), ref


# ---- 1. closed forms ------------------------------------------------------------------------------------------------------------------
def test_alphas_are_k_over_twenty():
    assert track.HOTA_ALPHAS == tuple(k / 20.0 for k in range(1, 20)) and len(track.HOTA_ALPHAS) == NA
    assert track.HOTA_ALPHAS[4] == 0.25 and track.HOTA_ALPHAS[9] == 0.5 and track.HOTA_ALPHAS[14] == 0.75
    assert track.HOTA_COUNTS == ("tp", "fn", "fp") and track.HOTA_SUMS == ("ass", "ass_re", "ass_pr", "loc") and track.HOTA_EPS == 2.0 ** -52


def test_a_perfect_tracker_scores_one_everywhere():
    fig, ref = summary(CRAFTED["PERFECT"])
    assert all(fig[k] == 1.0 for k in FIGURES + ("hota0", "loca0")), fig
    assert all(v == 1.0 for k in FIGURES for v in fig["per_alpha"][k]) and fig["per_alpha"]["alpha"] == list(track.HOTA_ALPHAS)
    assert ref["seq_hota_i"][0].tolist() == [[8, 0, 0]] * NA and fig["gt_dets"] == fig["hyp_dets"] == 8


def test_a_track_split_in_two_halves_assa():
    fig, ref = summary(CRAFTED["SPLIT"])
    assert fig["deta"] == 1.0 and fig["loca"] == 1.0 and fig["assa"] == 0.5 and abs(fig["hota"] - math.sqrt(0.5)) <= 1e-15
    assert fig["hota0"] == math.sqrt(0.5) and ref["hota_potential"][0, 0, :2].tolist() == [2.0, 2.0]
    assert ref["hota_id_count"][0, :2].tolist() == [2, 2] and ref["hota_gt_count"][0].tolist() == [4]


def test_an_object_found_in_half_of_its_frames():
    fig, _ = summary(CRAFTED["HALF_DETECTED"])
    assert fig["deta"] == 0.5 and fig["assa"] == 0.5 and fig["hota"] == 0.5 and fig["detpr"] == 1.0 and fig["detre"] == 0.5
    assert fig["assre"] == 0.5 and fig["asspr"] == 1.0 and fig["loca"] == 1.0


def test_two_objects_that_exchange_their_ids():
    """SWAP by hand.  Objects g = 0, 1 far apart over F = 4 frames, every box exact; ids (0, 1) in frames 0, 1 and (1, 0) in frames 2,
    3.  sim is 1 on the spatial pair and 0 across, so rs = cs = 1 and d = 1: every frame adds 1 to pot[g, the id on g]:
    pot[g, id] = 2 for all four (g, id).  gc = 4, ic = 4:  A = 2 / ((4 + 4) - 2) = 1/3 for every pair; the admissible pairs are the
    spatial ones, so every object is matched in every frame: tp = 8 at every threshold, DetA = 1.  matches[a, g, id] = 2 for all four
    pairs:  ass = 4 terms of 2 (2 / ((4 + 4) - 2)) = 4 (2/3) = 8/3, AssA = (8/3) / 8 = 1/3;  ass_re = 4 terms of 2 (2 / 4) = 4, AssRe =
    1/2, AssPr alike;  HOTA = sqrt(1/3)."""
    fig, ref = summary(CRAFTED["SWAP"])
    assert fig["deta"] == 1.0 and abs(fig["assa"] - 1.0 / 3.0) <= 1e-15 and abs(fig["hota"] - math.sqrt(1.0 / 3.0)) <= 1e-15
    assert fig["assre"] == 0.5 and fig["asspr"] == 0.5 and fig["loca"] == 1.0
    assert (ref["hota_potential"][0, :, :2] == 2.0).all() and (ref["hota_matches"][0, :, :, :2] == 2).all()
    assert ref["seq_hota_i"][0].tolist() == [[8, 0, 0]] * NA


def distractor_closed_form(fig, ref):
    assert fig["per_alpha"]["deta"] == [0.8] * 15 + [0.0] * 4 and fig["per_alpha"]["assa"] == [1.0] * 15 + [0.0] * 4
    assert ref["seq_hota_i"][0].tolist() == [[4, 0, 1]] * 15 + [[0, 4, 5]] * 4 and fig["per_alpha"]["loca"] == [0.75] * 15 + [1.0] * 4
    assert ref["hota_matches"][0, :15, 0, 0].tolist() == [4] * 15 and not ref["hota_matches"][0, :, 0, 1].any()


def test_the_global_score_keeps_the_track_against_a_better_box():
    fig, ref = summary(CRAFTED["DISTRACTOR"])
    distractor_closed_form(fig, ref)
    assert abs(ref["hota_potential"][0, 0, 0] - 24.0 / 7.0) <= 1e-15 and abs(ref["hota_potential"][0, 0, 1] - 4.0 / 7.0) <= 1e-15
    assert ref["hota_id_count"][0, :2].tolist() == [4, 1]


def exact_levels_closed_form(ref):
    tp = ref["seq_hota_i"][0, :, 0].tolist()
    assert tp == [3] * 5 + [2] * 5 + [1] * 5 + [0] * 4, tp                # 0.25, 0.5, 0.75 count AT alpha = 0.25, 0.5, 0.75


def test_the_thresholds_count_at_equality():
    case = CRAFTED["EXACT_LEVELS"]
    sims = [track.box_iou(case["gt"][0, g], case["boxes"][g, 0]) for g in range(3)]
    assert sims == [0.25, 0.5, 0.75]
    ref = reference(case)
    exact_levels_closed_form(ref)
    assert ref["seq_hota_f"][0, :, 3].tolist() == [1.5] * 5 + [1.25] * 5 + [0.75] * 5 + [0.0] * 4
    for g, levels in enumerate((5, 10, 15)):
        assert ref["hota_matches"][0, :, g, g].tolist() == [1] * levels + [0] * (NA - levels)


def test_planted_defects_of_the_reference_are_caught(monkeypatch):
    with monkeypatch.context() as m:                               # 1. the pair matched by its IoU alone
        m.setattr(track, "_hota_score", lambda A, sim: sim)
        fig, ref = summary(CRAFTED["DISTRACTOR"])
        assert ref["hota_matches"][0, 0, 0, 1] == 1                # frame 2 went to the better box
        with pytest.raises(AssertionError):
            distractor_closed_form(fig, ref)
    with monkeypatch.context() as m:                               # 2. > in place of >= at a threshold
        m.setattr(track, "_hota_levels", lambda sim: sum(1 for alpha in track.HOTA_ALPHAS if sim > alpha))
        with pytest.raises(AssertionError):
            exact_levels_closed_form(reference(CRAFTED["EXACT_LEVELS"]))
    with monkeypatch.context() as m:                               # 3. an epsilon at the threshold moves nothing here, but below it does
        m.setattr(track, "_hota_levels", lambda sim: sum(1 for alpha in track.HOTA_ALPHAS if sim >= alpha + 1e-12))
        with pytest.raises(AssertionError):
            exact_levels_closed_form(reference(CRAFTED["EXACT_LEVELS"]))
    distractor_closed_form(*summary(CRAFTED["DISTRACTOR"]))         # and the reference as it stands passes both
    exact_levels_closed_form(reference(CRAFTED["EXACT_LEVELS"]))


# ---- 2. an independent TrackEval-style evaluation -------------------------------------------------------------------------------------
def iou_matrix(gt, hyp):
    """[G, N] IoU of (left, top, width, height) boxes, vectorised float64"""
    gt, hyp = np.asarray(gt, np.float64), np.asarray(hyp, np.float64)
    l, t = np.maximum(gt[:, None, 0], hyp[None, :, 0]), np.maximum(gt[:, None, 1], hyp[None, :, 1])
    r = np.minimum(gt[:, None, 0] + gt[:, None, 2], hyp[None, :, 0] + hyp[None, :, 2])
    b = np.minimum(gt[:, None, 1] + gt[:, None, 3], hyp[None, :, 1] + hyp[None, :, 3])
    inter = np.clip(r - l, 0, None) * np.clip(b - t, 0, None)
    union = gt[:, None, 2] * gt[:, None, 3] + hyp[None, :, 2] * hyp[None, :, 3] - inter
    return inter / union


def trackeval_hota(case):
    """TrackEval's HOTA.eval_sequence and its final figures on one clean sequence: dense arrays, float scores, scipy's solver, a match
    counted at sim >= alpha - eps"""
    eps = np.finfo("float").eps
    alphas = np.arange(0.05, 0.99, 0.05)
    F, G = case["F"], case["G"]
    frames = []
    for f in range(F):
        n = int(case["n"][f])
        frames.append((np.arange(G), case["ids"][:n, f].astype(int), iou_matrix(case["gt"][f], case["boxes"][:n, f])))
    n_ids = int(max(i.max() for _, i, _ in frames if len(i))) + 1
    potential, gt_count, id_count = np.zeros((G, n_ids)), np.zeros((G, 1)), np.zeros((1, n_ids))
    for g_ids, t_ids, sim in frames:
        denom = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
        part = np.zeros_like(sim)
        mask = denom > 0 + eps
        part[mask] = sim[mask] / denom[mask]
        potential[g_ids[:, None], t_ids[None, :]] += part
        gt_count[g_ids] += 1
        id_count[0, t_ids] += 1
    score = potential / (gt_count + id_count - potential)
    tp, fn, fp, loc = np.zeros(len(alphas)), np.zeros(len(alphas)), np.zeros(len(alphas)), np.zeros(len(alphas))
    counts = [np.zeros((G, n_ids)) for _ in alphas]
    for g_ids, t_ids, sim in frames:
        if len(t_ids) == 0:
            fn += len(g_ids)
            continue
        rows, cols = linear_sum_assignment(-(score[g_ids[:, None], t_ids[None, :]] * sim))
        for a, alpha in enumerate(alphas):
            ok = sim[rows, cols] >= alpha - eps
            mr, mc = rows[ok], cols[ok]
            tp[a] += len(mr)
            fn[a] += len(g_ids) - len(mr)
            fp[a] += len(t_ids) - len(mr)
            loc[a] += sim[mr, mc].sum()
            counts[a][g_ids[mr], t_ids[mc]] += 1
    assa = np.zeros(len(alphas))
    for a in range(len(alphas)):
        c = counts[a]
        assa[a] = (c * (c / np.maximum(1, gt_count + id_count - c))).sum() / max(1, tp[a])
    deta = tp / np.maximum(1, tp + fn + fp)
    return dict(hota=float(np.mean(np.sqrt(deta * assa))), deta=float(np.mean(deta)), assa=float(np.mean(assa)))


def test_reference_agrees_with_a_trackeval_style_evaluation_on_thirty_seeded_cases():
    worst = dict(hota=0.0, deta=0.0, assa=0.0)
    splits = 0
    for seed in range(30):
        case = trackeval_case(seed)
        fig, ref = summary(case)
        want = trackeval_hota(case)
        for k in worst:
            worst[k] = max(worst[k], abs(fig[k] - want[k]))
        splits += int(ref["hota_id_count"][0, case["G"]:2 * case["G"]].any())
        assert 0.0 < fig["hota"] < 1.0 and fig["gt_dets"] == 30
    print("largest |reference - TrackEval style| over 30 cases: %r; cases with a split track: %d" % (worst, splits))
    assert splits >= 10
    assert all(v <= 1e-12 for v in worst.values()), worst


# ---- 3. the tie rule, the tables, sequences ---------------------------------------------------------------------------------------------
def test_a_profit_tie_is_decided_by_the_solvers_rule():
    case = CRAFTED["PROFIT_TIE"]
    ref = reference(case, return_matching=True)
    assert ref["hota_potential"][0, 0, 0] == ref["hota_potential"][0, 0, 1] > 0 and ref["hota_id_count"][0, :2].tolist() == [2, 2]
    rule = track.solve_assignment(np.full((2, track.MAX_SLOTS), 7, np.int64), np.arange(track.MAX_SLOTS)[None, :].repeat(2, 0) < 1)
    # (two rows that want column 0 alike: the row inserted second keeps it, the first falls back to its own column -- TIE_ONE_TRACK
    # of the optimal association)
    assert rule.tolist() == [-1, 0] and ref["hota_match"][:, 0].tolist() == [1, 1]
    assert ref["hota_matches"][0, 0, 0].tolist()[:2] == [0, 2] and ref["seq_hota_i"][0, 0].tolist() == [2, 0, 2]


def test_duplicate_ids_ids_beyond_the_table_nonfinite_boxes_and_empty_frames():
    ref = reference(CRAFTED["DUPLICATE_ID"], return_matching=True)
    assert ref["hota_id_count"][0, :2].tolist() == [4, 1] and ref["seq_hota_i"][0, 0].tolist() == [3, 0, 2]
    # frame 0: sims 1 and 8/12; rs = 1 + 2/3, both d = rs: the id adds (1 + 2/3) / rs = 1 in that frame, twice a term
    assert abs(ref["hota_potential"][0, 0, 0] - 3.0) <= 1e-15 and ref["hota_match"][:, 0].tolist() == [0, 0, 0]
    ref = reference(CRAFTED["ID_BEYOND"])
    assert ref["hota_potential"].shape == (1, 1, 4) and ref["hota_matches"].shape == (1, NA, 1, 4)
    assert ref["hota_id_count"][0].tolist() == [2, 0, 0, 0] and ref["seq_hota_i"][0, 0].tolist() == [2, 1, 3]       # 5 hypotheses, 3 gt
    assert ref["hota_potential"][0, 0, 0] == 2.0                   # an id beyond the table is in no row or column sum
    ref = reference(CRAFTED["NONFINITE"])
    # hypotheses: id 0 in frames 0, 2, 3, id 1 in frames 1, 2; slot 0 present in all four frames (a NaN left edge: present, IoU 0),
    # slot 1 in frames 0, 1, 2 (a NaN width is not > 0); matched: (0, id 0) in frames 0 and 3, (1, id 1) in frames 1 and 2
    assert ref["seq_hota_i"][0, 0].tolist() == [4, 3, 1] and ref["hota_id_count"][0, :2].tolist() == [3, 2]
    assert ref["hota_gt_count"][0].tolist() == [4, 3]
    ref = reference(CRAFTED["EMPTY_FRAMES"])
    assert ref["seq_hota_i"][0, 0].tolist() == [1, 1, 1] and ref["hota_gt_count"][0].tolist() == [2] and ref["hota_id_count"][0, 0] == 2
    fig, ref = summary(CRAFTED["NOTHING"])
    assert not ref["seq_hota_i"].any() and all(math.isnan(fig[k]) for k in FIGURES + ("hota0", "loca0"))
    assert all(math.isnan(v) for v in fig["per_alpha"]["hota"]) and fig["gt_dets"] == fig["hyp_dets"] == 0


def test_sequences_are_scored_on_their_own_and_the_summary_adds_them():
    a, b = hota_case(3, 1, 5, 2, seed=1), hota_case(3, 1, 5, 2, seed=2)
    both, ra, rb = reference(stack([a, b])), reference(a), reference(b)
    for k in ra:
        assert np.array_equal(both[k], np.concatenate([ra[k], rb[k]])), k
    assert both["seq_hota_i"][:, 0, 0].min() > 0
    fig = track.hota_summary(both["seq_hota_i"].sum(0), both["seq_hota_f"].sum(0))
    ti, tf = ra["seq_hota_i"][0].astype(np.int64) + rb["seq_hota_i"][0], ra["seq_hota_f"][0] + rb["seq_hota_f"][0]
    for a_ in range(NA):
        tp, fn, fp = (int(v) for v in ti[a_])
        assert fig["per_alpha"]["deta"][a_] == tp / max(1, tp + fn + fp) and fig["per_alpha"]["assa"][a_] == tf[a_, 0] / max(1, tp)
        assert fig["per_alpha"]["hota"][a_] == math.sqrt(fig["per_alpha"]["deta"][a_] * fig["per_alpha"]["assa"][a_])
    assert fig["hota"] == sum(fig["per_alpha"]["hota"]) / NA and fig["hota0"] == fig["per_alpha"]["hota"][0]


def test_a_smaller_table_ignores_the_ids_beyond_it():
    case = hota_case(6, 2, 7, 3, seed=5)
    full = reference(case)
    small = track.reference_hota(case["boxes"], case["n"], case["ids"], case["gt"], 7, n_ids=9)
    assert small["hota_id_count"].shape == (2, 9) and case["ids"].max() >= 9
    cut = dict(case, ids=np.where(case["ids"] >= 9, 10 ** 6, case["ids"]))
    again = track.reference_hota(cut["boxes"], cut["n"], cut["ids"], cut["gt"], 7, n_ids=9)
    for k in small:
        assert np.array_equal(small[k], again[k]), k
    assert (small["seq_hota_i"][:, :, 0] + small["seq_hota_i"][:, :, 2] == full["seq_hota_i"][:, :, 0] + full["seq_hota_i"][:, :, 2]).all()


# ---- 4. the summary's conventions, the refusals, the prototype --------------------------------------------------------------------------
def test_summary_conventions():
    ti, tf = np.zeros((NA, 3), np.int64), np.zeros((NA, 4))
    ti[:, 1] = 5                                                   # ground truth and no hypothesis: tp = 0
    fig = track.hota_summary(ti, tf)
    assert fig["deta"] == fig["assa"] == fig["hota"] == fig["detre"] == fig["detpr"] == 0.0 and fig["loca"] == 1.0 and fig["loca0"] == 1.0
    ti[:, 1], ti[:, 2] = 0, 3                                      # hypotheses and no ground truth
    fig = track.hota_summary(ti, tf)
    assert fig["deta"] == 0.0 and fig["loca"] == 1.0 and fig["gt_dets"] == 0 and fig["hyp_dets"] == 3
    ti[:] = 0
    assert all(math.isnan(track.hota_summary(ti, tf)[k]) for k in FIGURES)
    ti[:, 0], tf[:, 0], tf[:, 3] = 2, 1.0, 1.5
    fig = track.hota_summary(ti.tolist(), tf.tolist())
    assert fig["deta"] == 1.0 and fig["assa"] == 0.5 and fig["loca"] == 0.75 and fig["hota0"] == math.sqrt(0.5)
    with pytest.raises(ValueError, match="hota_summary"):
        track.hota_summary(ti[:5], tf)


def test_reference_refusals():
    c = hota_case(3, 2, 4, 2, seed=3)
    args = (c["boxes"], c["n"], c["ids"], c["gt"])
    with pytest.raises(ValueError, match="ground-truth slots"):
        track.reference_hota(c["boxes"], c["n"], c["ids"], np.zeros((8, 9, 4), np.float32), 4)
    with pytest.raises(ValueError, match="not sequences of"):
        track.reference_hota(*args, 3)
    with pytest.raises(ValueError, match="not sequences of"):
        track.reference_hota(c["boxes"], c["n"], c["ids"], c["gt"][:4], 4)
    for n_ids in (0, track.MAX_IDS + 1):
        with pytest.raises(ValueError, match="n_ids must be within"):
            track.reference_hota(*args, 4, n_ids=n_ids)
    with pytest.raises(ValueError, match="objects per frame"):
        track.reference_hota(np.zeros((33, 1, 4), np.float32), np.zeros(1), np.zeros((33, 1)), np.zeros((1, 1, 4), np.float32), 1)
    with pytest.raises(ValueError, match="more than 2\\^31 - 1"):
        big = 600
        track.reference_hota(np.zeros((1, big * 2, 4), np.float32), np.zeros(big * 2), np.zeros((1, big * 2)),
                             np.zeros((big * 2, 8, 4), np.float32), 2, n_ids=track.MAX_IDS)
    assert track.reference_hota(*args, 4)["hota_potential"].shape == (2, 2, 12)        # n_ids = None: F T
    assert not hasattr(track.StreamTracker, "hota")                # out of scope on a stream


def test_header_prototype_ctypes_row_and_argument_count_agree():
    header = (ROOT / "include" / "air_hip.h").read_text()
    m = re.search(r"AIR_ENGINE_API int air_track_hota\(([^;]*?)\);", header, re.S)
    assert m, "air_track_hota is not declared in include/air_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float *boxes", "const int *num_objects", "const int *track_id", "const float *gt_boxes", "int T", "int G",
                      "int S", "int F", "int R", "int n_ids", "double *potential", "int *id_count", "int *gt_count", "int *matches",
                      "int *seq_hota_i", "double *seq_hota_f", "void *stream"]
    restype, argtypes = _lib.SIGNATURES["air_track_hota"]
    assert restype is _lib.c_int and len(argtypes) == len(params) == 17
    for p, t in zip(params, argtypes):
        assert (t is _lib.c_int) == ("*" not in p), p
    source = (ROOT / "attend_infer_repeat_amd" / "csrc" / "track_kernels.hip").read_text()
    m = re.search(r'extern "C" int air_track_hota\(([^)]*)\)', source)
    assert m and [" ".join(p.split()) for p in m.group(1).split(",")] == params
    assert "HOTA" in track.__doc__ and "alpha_k = k / 20.0" in track.__doc__ and "air_track_hota" in header
