"""Host-side tests of the optimal association and the IDF1 metric (attend_infer_repeat_amd/track.py): `solve_assignment` against
scipy's exact optimum and against brute force, the stated tie rule, `reference_associate(matching="optimal")` on the worked example,
the chain and random sequences, `reference_identity` against brute force, scipy and known answers, the refusals and the ABI.  No GPU."""
import itertools
import math
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from test_track_host import BOX, OUTPUTS, _overflow_frames, associate, build_rows, crafted_rows
from track_optimal_cases import CHAIN, TIE_ONE_TRACK, TIE_TWO_TRACKS, WORKED, identity_case, planted

from attend_infer_repeat_amd import track
from attend_infer_repeat_amd.tile import box_iou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def value(profit, admissible, col):
    """the summed profit of an assignment, after checking that it is one: admissible pairs, a column taken once"""
    taken = [int(c) for c in col if c >= 0]
    assert len(set(taken)) == len(taken) and all(admissible[i, c] for i, c in enumerate(col) if c >= 0)
    return sum(int(profit[i, c]) for i, c in enumerate(col) if c >= 0)


def scipy_optimum(profit, admissible):
    """the exact optimum by scipy on the augmented matrix: every row's own column of profit 0 behind the m real ones"""
    n, m = profit.shape
    if n == 0:
        return 0
    aug = np.full((n, m + n), -np.inf)
    aug[:, :m] = np.where(admissible, profit.astype(np.float64), -np.inf)
    aug[np.arange(n), m + np.arange(n)] = 0.0
    rows, cols = linear_sum_assignment(aug, maximize=True)
    return int(aug[rows, cols].sum())


def brute_force(profit, admissible):
    """(the optimum, the assignments that attain it) over all partial injections of rows into admissible columns"""
    n, m = profit.shape
    best, argbest = -1, []
    for col in itertools.product(range(-1, m), repeat=n):
        taken = [c for c in col if c >= 0]
        if len(set(taken)) != len(taken) or any(c >= 0 and not admissible[i, c] for i, c in enumerate(col)):
            continue
        v = sum(int(profit[i, c]) for i, c in enumerate(col) if c >= 0)
        if v > best:
            best, argbest = v, []
        if v == best:
            argbest.append(col)
    return best, argbest


# ---- solve_assignment ---------------------------------------------------------------------------------------------------------------
def test_solver_attains_the_exact_optimum_of_scipy():
    rng = np.random.default_rng(0)
    for case in range(2000):
        n, m = (int(v) for v in rng.integers(1, 33, 2)) if case % 4 else (int(rng.integers(1, 9)), int(rng.integers(1, 9)))
        density = rng.uniform(0.1, 1.0)
        admissible = rng.uniform(size=(n, m)) < density
        if case % 5 == 0:                                          # repeated profits
            profit = rng.integers(1, 4, (n, m)).astype(np.int64)
        elif case % 5 == 1:                                        # the kernel's range: 1 .. 1 + 2^32
            profit = 1 + rng.integers(0, 2 ** 32 + 1, (n, m)).astype(np.int64)
        else:
            profit = rng.integers(1, 1000, (n, m)).astype(np.int64)
        if case % 7 == 0:                                          # empty rows and empty columns
            admissible[rng.integers(n)] = False
            admissible[:, rng.integers(m)] = False
        col = track.solve_assignment(profit, admissible)
        assert col.shape == (n,) and value(profit, admissible, col) == scipy_optimum(profit, admissible), case
    assert 33 * (2 ** 32 + 1) < 2 ** 53                            # scipy's float sums were exact


def test_solver_assignment_is_the_brute_force_optimum_where_that_is_unique():
    rng = np.random.default_rng(1)
    unique = 0
    for case in range(600):
        n, m = (int(v) for v in rng.integers(1, 5, 2))
        admissible = rng.uniform(size=(n, m)) < rng.uniform(0.3, 1.0)
        profit = rng.integers(1, 6 if case % 2 else 1000, (n, m)).astype(np.int64)
        best, argbest = brute_force(profit, admissible)
        col = track.solve_assignment(profit, admissible)
        assert value(profit, admissible, col) == best and tuple(col) in argbest
        if len(argbest) == 1:
            unique += 1
            assert tuple(col) == argbest[0]
    assert unique >= 200
    assert track.solve_assignment(np.zeros((0, 3), np.int64), np.zeros((0, 3), bool)).shape == (0,)
    assert track.solve_assignment(np.ones((2, 3), np.int64), np.zeros((2, 3), bool)).tolist() == [-1, -1]


def test_solver_planted_ties_follow_the_stated_rule():
    one, yes = np.ones((1, 3), np.int64), np.ones((1, 3), bool)
    assert track.solve_assignment(5 * one, yes).tolist() == [0]                               # equal: the lowest column
    assert track.solve_assignment(5 * one, np.array([[False, True, True]])).tolist() == [1]
    # two rows, one column, equal profits: the row inserted second takes it -- the first row's own column, the lower of two equal
    # columns, is where the path ends (track_optimal_cases.TIE_ONE_TRACK derives it)
    assert track.solve_assignment([[5], [5]], [[True], [True]]).tolist() == [-1, 0]
    # all four pairs alike: nothing moves, each row takes the lowest column still free
    assert track.solve_assignment([[5, 5], [5, 5]], np.ones((2, 2), bool)).tolist() == [0, 1]
    assert track.solve_assignment(np.full((3, 3), 7), np.ones((3, 3), bool)).tolist() == [0, 1, 2]
    # row 1 can only take column 0, which row 0 holds at no loss against column 1: row 0 moves on (the optimum is unique)
    assert track.solve_assignment([[5, 5], [5, 0]], [[True, True], [True, False]]).tolist() == [1, 0]
    # an admissible pair always beats staying unmatched (profit >= 1), however many rows are rerouted for it
    assert track.solve_assignment([[9, 1], [9, 0]], [[True, True], [True, False]]).tolist() == [1, 0]


# ---- reference_associate(matching="optimal") ------------------------------------------------------------------------------------------
def test_worked_example_greedy_leaves_a_birth_optimal_matches_both():
    iou = {d: box_iou(BOX(0.0), BOX(float(d))) for d in (3, 5, 6, 14)}
    assert iou[3] == 7.0 / 13.0 and iou[5] == 5.0 / 15.0 and iou[6] == 0.25 and iou[14] == 0.0
    assert iou[5] + iou[6] > iou[3]                                # 0.583 in total against 0.538
    M, B, U = track.MATCHED, track.BORN, track.UNCONFIRMED
    _, g = planted(WORKED, "greedy")
    assert g["track_id"].T.tolist() == [[0, 1], [0, 2]] and g["obj_state"].T.tolist() == [[B, B], [M, B]]
    assert g["prev_frame"][:, 1].tolist() == [0, -1] and g["prev_slot"][:, 1].tolist() == [0, -1]
    assert g["affinity"][:, 1].tolist() == [np.float32(7.0 / 13.0), 0.0]
    assert g["num_tracks"].tolist() == [3] and g["track_first"][0, :3].tolist() == [0, 0, 1]
    assert g["track_last"][0, :3].tolist() == [1, 0, 1] and g["track_length"][0, :3].tolist() == [2, 1, 1]   # B coasts: last seen in 0
    assert g["track_gaps"][0, :3].tolist() == [0, 0, 0] and g["state_counts"][0].tolist() == [0, 1, 3, 0, 0, 0]
    _, o = planted(WORKED, "optimal")
    assert o["track_id"].T.tolist() == [[0, 1], [1, 0]] and o["obj_state"].T.tolist() == [[B, B], [M, M]]
    assert o["prev_frame"][:, 1].tolist() == [0, 0] and o["prev_slot"][:, 1].tolist() == [1, 0]
    assert o["affinity"][:, 1].tolist() == [np.float32(1.0 / 3.0), np.float32(0.25)]
    assert o["num_tracks"].tolist() == [2] and o["track_first"][0].tolist() == [0, 0, -1, -1]                # no birth in frame 1
    assert o["track_last"][0].tolist() == [1, 1, -1, -1] and o["track_length"][0].tolist() == [2, 2, 0, 0]
    assert o["track_gaps"][0].tolist() == [0, 0, 0, 0] and o["state_counts"][0].tolist() == [0, 2, 2, 0, 0, 0]
    assert U not in o["obj_state"]


def test_chain_the_third_object_reroutes_the_first_two():
    M, B = track.MATCHED, track.BORN
    _, g = planted(CHAIN, "greedy")
    assert g["track_id"][:, 1].tolist() == [0, 1, 3] and g["obj_state"][:, 1].tolist() == [M, M, B]
    case, o = planted(CHAIN, "optimal")
    assert o["track_id"][:, 1].tolist() == [1, 2, 0] and o["obj_state"][:, 1].tolist() == [M, M, M]
    assert o["prev_slot"][:, 1].tolist() == [1, 2, 0] and o["num_tracks"].tolist() == [3]
    assert o["affinity"][:, 1].tolist() == [np.float32(6.0 / 14.0), np.float32(6.0 / 14.0), np.float32(7.0 / 13.0)]
    # the solver on the frame's table: after two insertions rows 0 and 1 hold columns 0 and 1; the third moves both
    profit, admissible = np.zeros((3, 32), np.int64), np.zeros((3, 32), bool)
    for j, k, aff in ((0, 0, 8 / 12), (0, 1, 6 / 14), (1, 1, 8 / 12), (1, 2, 6 / 14), (2, 0, 7 / 13)):
        profit[j, k], admissible[j, k] = 1 + math.floor(aff * 2.0 ** 32), True
    assert track.solve_assignment(profit[:2], admissible[:2]).tolist() == [0, 1]
    assert track.solve_assignment(profit, admissible).tolist() == [1, 2, 0]


def test_planted_ties_in_the_association():
    M, B = track.MATCHED, track.BORN
    _, o = planted(TIE_ONE_TRACK, "optimal")
    assert o["track_id"][:, 1].tolist() == [1, 0] and o["obj_state"][:, 1].tolist() == [B, M]
    _, g = planted(TIE_ONE_TRACK, "greedy")
    assert g["track_id"][:, 1].tolist() == [0, 1] and g["obj_state"][:, 1].tolist() == [M, B]
    _, o = planted(TIE_TWO_TRACKS, "optimal")
    assert o["track_id"][:, 1].tolist() == [0, 1] and o["obj_state"][:, 1].tolist() == [M, M]


@pytest.mark.parametrize("T,A,S,F,kw", [(3, 5, 3, 5, {}), (6, 4, 2, 9, dict(iou_gate=0.2, appearance_weight=0.6, birth_score=0.4, max_age=2)),
                                        (12, 3, 2, 6, dict(iou_gate=0.05, appearance_weight=0.0)), (32, 2, 1, 4, dict(iou_gate=0.0))])
def test_every_frame_of_the_optimal_reference_attains_the_scipy_optimum(monkeypatch, T, A, S, F, kw):
    case, _ = crafted_rows(T, A, S, F, seed=T + F, margin=0.0, **kw)            # (host only: no margin to keep)
    tables = []
    solve = track.solve_assignment

    def recording(profit, admissible):
        col = solve(profit, admissible)
        tables.append((profit.copy(), admissible.copy(), col.copy()))
        return col

    monkeypatch.setattr(track, "solve_assignment", recording)
    out = track.reference_associate(case["what"], case["boxes"], case["score"], case["n"], F, matching="optimal", **kw)
    assert tables and any(a.sum() > 1 for _, a, _ in tables)
    for profit, admissible, col in tables:                         # the table the reference held at that frame
        assert profit.shape[1] == 32 and (profit[admissible] >= 1).all() and (profit[admissible] <= 1 + 2 ** 32).all()
        assert value(profit, admissible, col) == scipy_optimum(profit, admissible)
    assert sum(int((c >= 0).sum()) for _, _, c in tables) == int(out["state_counts"][:, track.MATCHED].sum())
    assert (out["state_counts"].sum(1) == T * F).all()


def frame_profit(out, r, w, what, boxes, prev_rows):
    """the summed profit of frame r's matches in an answer of reference_associate"""
    total = 0
    for j in range(out["track_id"].shape[0]):
        if out["obj_state"][j, r] != track.MATCHED:
            continue
        pr, pj = prev_rows + int(out["prev_frame"][j, r]), int(out["prev_slot"][j, r])
        d = what[pj, pr].astype(np.float64) - what[j, r].astype(np.float64)
        msd = np.cumsum(d * d)[-1] / np.float64(len(d))
        aff = (1.0 - w) * box_iou(boxes[pj, pr], boxes[j, r]) + w / (1.0 + float(msd))
        assert out["affinity"][j, r] == np.float32(aff)
        total += 1 + math.floor(aff * 2.0 ** 32)
    return total


def test_optimal_beats_or_equals_greedy_on_the_first_frame_that_can_differ():
    better = 0
    for seed in range(40):                                         # crowded frames: eight boxes of side 10 within 25 pixels
        rng = np.random.default_rng(100 + seed)
        T, A, S, w = 8, 3, 2, 0.3
        what, score = rng.normal(size=(T, 2 * S, A)).astype(np.float32), np.ones((T, 2 * S), np.float32)
        boxes = np.concatenate([rng.uniform(0, 25, (T, 2 * S, 2)), rng.uniform(8, 12, (T, 2 * S, 2))], -1).astype(np.float32)
        args = (what, boxes, score, rng.integers(3, T + 1, 2 * S).astype(np.int32), 2)
        o, g = (track.reference_associate(*args, iou_gate=0.05, appearance_weight=w, matching=m) for m in ("optimal", "greedy"))
        for s in range(S):                                         # frame 0 holds births only: the same table in frame 1
            assert all(np.array_equal(o[k][:, 2 * s], g[k][:, 2 * s]) for k in ("track_id", "obj_state"))
            po, pg = (frame_profit(x, 2 * s + 1, w, what, boxes, 2 * s) for x in (o, g))
            assert po >= pg
            better += po > pg
    print("optimal strictly better in", better, "of 80 frames")
    assert better >= 1                                             # (the frames are crowded enough for the two rules to part)


def test_greedy_is_the_default_and_unchanged():
    case, ref = crafted_rows(6, 5, 3, 5, seed=4)
    args = (case["what"], case["boxes"], case["score"], case["n"], 5)
    a, b = track.reference_associate(*args, return_margins=True), track.reference_associate(*args, return_margins=True, matching="greedy")
    assert sorted(a) == sorted(b) == sorted(OUTPUTS + ("gate_margin", "round_margin"))
    for k in a:
        assert a[k].dtype == b[k].dtype == ref[k].dtype and np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], ref[k]), k
    o = track.reference_associate(*args, return_margins=True, matching="optimal")
    assert sorted(o) == sorted(OUTPUTS + ("gate_margin",)) and np.array_equal(o["gate_margin"][:1], a["gate_margin"][:1])


def test_nonfinite_overflow_coasting_and_tiny_affinities_under_the_optimal_rule():
    nan = float("nan")
    # a non-finite object takes no part: the finite one behind it continues the track
    out = associate([[(BOX(0.0), 0.9, 1.0)], [((1.0, nan, 10.0, 10.0), 0.9, 1.0), (BOX(1.0), 0.9, 1.0)]], 2, 2, matching="optimal")
    assert out["obj_state"][:, 1].tolist() == [track.NONFINITE, track.MATCHED] and out["track_id"][:, 1].tolist() == [-1, 0]
    out = associate([[(BOX(0.0), 0.9, 1.0)], [(BOX(1.0), nan, 1.0)]], 1, 2, matching="optimal")
    assert out["obj_state"][0].tolist() == [track.BORN, track.NONFINITE]
    # OVERFLOW: 32 coasting tracks hold every slot, as under the greedy rule (nothing is admissible: the answers are the same)
    for F, max_age in ((4, 1), (3, 0)):
        what, boxes, score, n = build_rows(_overflow_frames(F), 32, 3)
        o, g = (track.reference_associate(what, boxes, score, n, F, max_age=max_age, matching=m) for m in ("optimal", "greedy"))
        assert o["state_counts"][0, track.OVERFLOW] == 32 * (F - 2) and all(np.array_equal(o[k], g[k]) for k in OUTPUTS)
    # max_age coasting: back under its id after one missing frame, a new id after two
    out = associate([[(BOX(0.0), 0.9, 1.0)], [], [(BOX(1.0), 0.9, 1.0)]], 2, 3, max_age=1, matching="optimal")
    assert out["track_id"][0].tolist() == [0, -1, 0] and out["track_gaps"][0, 0] == 1 and out["prev_frame"][0, 2] == 0
    out = associate([[(BOX(0.0), 0.9, 1.0)], [], [], [(BOX(0.0), 0.9, 1.0)]], 1, 4, max_age=1, matching="optimal")
    assert out["track_id"][0].tolist() == [0, -1, -1, 1]
    # matching ignores birth_score
    out = associate([[(BOX(0.0), 0.9, 1.0)], [(BOX(1.0), 0.1, 1.0)]], 1, 2, matching="optimal")
    assert out["obj_state"][0].tolist() == [track.BORN, track.MATCHED]
    # aff < 2^-32: profit 1, still a match.  iou_gate 0, w = 1e-12: a sliver of overlap and a what row far away
    frames = [[((0.0, 0.0, 10.0, 10.0), 0.9, 0.0)], [((9.9999, 9.9999, 10.0, 10.0), 0.9, 1e6)]]
    out = associate(frames, 1, 2, iou_gate=0.0, appearance_weight=1.0 - 1e-12, matching="optimal")
    aff = float(out["affinity"][0, 1])
    assert 0.0 < aff < 2.0 ** -32 and math.floor(aff * 2.0 ** 32) == 0
    assert out["obj_state"][0].tolist() == [track.BORN, track.MATCHED] and out["track_id"][0].tolist() == [0, 0]


# ---- reference_identity -------------------------------------------------------------------------------------------------------------
def idtp_brute_force(overlap):
    G, n = overlap.shape
    ids = [i for i in range(n) if overlap[:, i].any()]
    best = 0
    for pick in itertools.product([-1] + ids, repeat=G):
        used = [i for i in pick if i >= 0]
        if len(set(used)) == len(used):
            best = max(best, sum(int(overlap[g, i]) for g, i in enumerate(pick) if i >= 0))
    return best


def identity(case, tau=0.5, n_ids=None):
    return track.reference_identity(case["boxes"], case["n"], case["ids"], case["gt"], case["F"], tau, n_ids)


def test_identity_idtp_is_brute_force_and_scipy():
    for seed in range(12):                                         # G <= 4, ids <= 6
        case = identity_case(2, 2, 3, 1 + seed % 4, seed)
        out = identity(case)
        assert out["overlap"].shape == (2, case["G"], 6) and out["overlap"].dtype == out["seq_idf"].dtype == np.int32
        for s in range(2):
            assert out["seq_idf"][s, 0] == idtp_brute_force(out["overlap"][s])
            assert out["seq_idf"][s, 3] == out["overlap"][s].any(0).sum()
    hits = 0
    for seed in range(6):                                          # G = 8, up to 200 ids
        case = identity_case(8, 2, 25, 8, 50 + seed, fresh_ids=bool(seed % 2))
        out = identity(case, tau=0.3)
        assert out["overlap"].shape == (2, 8, 200)
        for s in range(2):
            rows, cols = linear_sum_assignment(out["overlap"][s].astype(np.float64), maximize=True)
            assert out["seq_idf"][s, 0] == out["overlap"][s][rows, cols].sum()
            hits += int(out["seq_idf"][s, 0])
        r = np.arange(50)                                          # the counts of the definition, restated
        n = np.clip(case["n"], 0, 8)
        hyp = (case["ids"] >= 0) & np.isfinite(case["boxes"]).all(-1) & (np.arange(8)[:, None] < n[None, :])
        assert out["seq_idf"][:, 2].tolist() == hyp.reshape(8, 2, 25).sum((0, 2)).tolist()
        assert out["seq_idf"][:, 1].tolist() == (case["gt"][..., 2] > 0).reshape(2, 25, 8).sum((1, 2)).tolist() and len(r) == 50
    assert hits > 100


def one_object(ids, F=10):
    boxes = np.tile(np.array(BOX(5.0), np.float32), (1, F, 1))
    return dict(boxes=boxes, n=np.ones(F, np.int32), ids=np.array([ids], np.int32), gt=boxes[0][:, None, :].copy(), T=1, S=1, F=F, G=1)


def test_identity_known_answers():
    out = identity(one_object([0] * 10))                           # perfect tracking
    assert out["seq_idf"].tolist() == [[10, 10, 10, 1]] and track.idf_summary(out["seq_idf"][0])["idf1"] == 1.0
    out = identity(one_object([0] * 6 + [1] * 4))                  # one object under id 0 for 6 frames and id 1 for 4
    assert out["seq_idf"].tolist() == [[6, 10, 10, 2]] and out["overlap"][0, 0].tolist() == [6, 4] + [0] * 8
    fig = track.idf_summary(out["seq_idf"][0])
    assert fig == dict(idf1=0.6, idp=0.6, idr=0.6, idtp=6, idfp=4, idfn=4, gt_frames=10, hyp_frames=10)
    case = one_object([-1] * 10)                                   # no hypotheses
    fig = track.idf_summary(identity(case)["seq_idf"][0])
    assert fig["idr"] == 0.0 and math.isnan(fig["idp"]) and fig["idf1"] == 0.0 and fig["hyp_frames"] == 0
    case = one_object([0] * 10)                                    # no ground truth
    case["gt"][:] = 0
    fig = track.idf_summary(identity(case)["seq_idf"][0])
    assert fig["idp"] == 0.0 and math.isnan(fig["idr"]) and fig["gt_frames"] == 0
    case["ids"][:] = -1                                            # neither
    fig = track.idf_summary(identity(case)["seq_idf"][0])
    assert all(math.isnan(fig[k]) for k in ("idf1", "idp", "idr")) and fig["idtp"] == fig["idfp"] == fig["idfn"] == 0


def test_identity_duplicated_ids_ids_out_of_range_and_the_strict_threshold():
    F = 3
    boxes = np.tile(np.array(BOX(5.0), np.float32), (2, F, 1))
    case = dict(boxes=boxes, n=np.full(F, 2, np.int32), ids=np.array([[0, 0, 1], [0, 1, 5]], np.int32),
                gt=boxes[0][:, None, :].copy(), T=2, S=1, F=F, G=1)
    out = identity(case)                                           # id 0 twice in frame 0: once per hypothesis
    assert out["overlap"][0, 0].tolist() == [3, 2, 0, 0, 0, 1] and out["seq_idf"].tolist() == [[3, 3, 6, 3]]
    out = identity(case, n_ids=5)                                  # id 5 is ignored in the table, still a hypothesis
    assert out["overlap"].shape == (1, 1, 5) and out["overlap"][0, 0].tolist() == [3, 2, 0, 0, 0]
    assert out["seq_idf"].tolist() == [[3, 3, 6, 2]]
    assert identity(case, tau=1.0)["seq_idf"].tolist() == [[0, 3, 6, 0]]                     # IoU 1 is not > 1
    case["n"][:] = [1, 7, -3]                                      # counts are clipped to 0..T
    assert identity(case)["seq_idf"].tolist() == [[2, 3, 3, 2]]


# ---- refusals and the ABI -----------------------------------------------------------------------------------------------------------
def test_the_new_refusals():
    for bad in ("hungarian", None, "", "Optimal", 1):
        with pytest.raises(ValueError, match="matching must be one of"):
            track.check_arguments(3, 5, 15, matching=bad)
    assert track.check_arguments(3, 5, 15, matching="optimal") == track.check_arguments(3, 5, 15) == (3, 5, 3)
    case, _ = crafted_rows(3, 2, 1, 2, seed=1)
    with pytest.raises(ValueError, match="matching"):
        track.reference_associate(case["what"], case["boxes"], case["score"], case["n"], 2, matching="best")
    idc = one_object([0] * 4, F=4)
    for n_ids in (0, -1, 32768):
        with pytest.raises(ValueError, match="n_ids"):
            identity(idc, n_ids=n_ids)
    with pytest.raises(ValueError, match="tau"):
        identity(idc, tau=1.5)
    with pytest.raises(ValueError, match="ground-truth slots"):
        track.reference_identity(idc["boxes"], idc["n"], idc["ids"], np.zeros((4, 9, 4), np.float32), 4)
    with pytest.raises(ValueError, match="frames"):
        track.reference_identity(idc["boxes"], idc["n"], idc["ids"], idc["gt"], 3)


def header_arguments(header):
    """{entry: the parameter declarations of its prototype in include/air_hip.h, in order} of the ten entries track.py launches"""
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    args = {}
    for name in ("associate", "associate_optimal", "associate_motion", "associate_motion_gated", "associate_stream", "owner", "score",
                 "score_stream", "idf", "hota"):
        m = re.search(r"AIR_ENGINE_API int air_track_%s\(([^;]*)\);" % name, src)
        assert m, name
        args["air_track_" + name] = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    return args


def test_abi_numbers_header_and_ctypes_table():
    import ctypes

    from attend_infer_repeat_amd import _lib
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5
    header = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    assert re.search(r"#define\s+AIR_ABI_VERSION\s+10\b", header) and re.search(r"#define\s+AIR_ENGINE_ABI_VERSION\s+5\b", header)
    args = header_arguments(header)
    assert set(args) == set(track.ENTRY_ARGS) and len(args) == 10                            # every air_track_* entry track.py launches
    for name in args:
        assert len(args[name]) == len(_lib.SIGNATURES[name][1]) and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        for text, ctype in zip(args[name], _lib.SIGNATURES[name][1]):
            want = _lib.P if "*" in text else (ctypes.c_double if text.startswith("double") else ctypes.c_int)
            assert ctype is want, (name, text)
        names = [re.search(r"(\w+)$", text).group(1) for text in args[name]]
        assert names[-1] == "stream" and tuple(names[:-1]) == track.ENTRY_ARGS[name], name   # the launch tuples: the header's order
    assert args["air_track_associate_optimal"] == args["air_track_associate"]                # exactly its argument list
    assert len(args["air_track_idf"]) == 14 and args["air_track_idf"][10] == "int n_ids"


# ---- the launch list is built from the header's names -------------------------------------------------------------------------------
class Named:
    """a stand-in for a device buffer that knows the name it was made under"""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<%s>" % self.name


def stub_tracker(matching, motion, motion_gate):
    """a SequenceTracker without its constructor: every buffer a Named, a library whose entries are their own names, p = identity"""
    import types
    tk = object.__new__(track.SequenceTracker)
    lib = types.SimpleNamespace(**{name: name for name in track.ENTRY_ARGS})
    tk._H = types.SimpleNamespace(lib=lambda: lib, _p=lambda t: t)
    tk.provider = types.SimpleNamespace(**{k: Named("provider." + k) for k in ("boxes", "score", "num_objects", "owner")})
    tk._what, tk._rows = Named("rows.what"), {"where": Named("rows.where")}
    tk.T, tk.S, tk.F, tk.R, tk.A, tk.img_size = 3, 2, 5, 10, 7, (48, 50)
    tk.iou_gate, tk.appearance_weight, tk.birth_score, tk.max_age, tk.matching = 0.125, 0.25, 0.5, 2, matching
    tk.motion, tk.motion_gate = motion, motion_gate
    for k in track._PER_OBJECT + track._TABLES + ("track_owner", "pred_where", "pred_boxes", "pred_d2"):
        setattr(tk, k, Named(k))
    tk._build_plan()
    return tk


@pytest.mark.parametrize("matching,motion,gate,entry", [("greedy", False, None, "air_track_associate"),
                                                        ("optimal", False, None, "air_track_associate_optimal"),
                                                        ("greedy", True, None, "air_track_associate_motion"),
                                                        ("optimal", True, None, "air_track_associate_motion"),
                                                        ("optimal", True, 9.5, "air_track_associate_motion_gated")])
def test_the_built_plan_files_every_value_under_the_headers_name(matching, motion, gate, entry):
    noise = dict(process_noise=(1e-3, 2e-3), measurement_noise=3e-3, velocity_var=4e-2)
    tk = stub_tracker(matching, noise if motion else None, gate)
    assert list(tk.segments) == ["associate", "owner"] and [e[2] for e in tk._plan] == [entry, "air_track_owner"]
    assert all(fn == name for fn, _, name in tk._plan)             # the library's entry of that name
    header = header_arguments(open(os.path.join(ROOT, "include", "air_hip.h")).read())
    scalars = dict(T=3, S=2, F=5, R=10, A=7, H=48, W=50, iou_gate=0.125, appearance_weight=0.25, birth_score=0.5, max_age=2,
                   matching=track.MATCHINGS.index(matching), q_shift=1e-3, q_scale=2e-3, measurement_noise=3e-3, velocity_var=4e-2,
                   gate_d2=gate)
    buffers = dict(what=tk._what, where=tk._rows["where"], boxes=tk.provider.boxes, score=tk.provider.score,
                   num_objects=tk.provider.num_objects, owner=tk.provider.owner)
    for _, got, name in tk._plan:
        names = [re.search(r"(\w+)$", text).group(1) for text in header[name]][:-1]
        assert len(got) == len(names), name
        for n, v in zip(names, got):
            if n in scalars:
                assert v == scalars[n] and type(v) is type(scalars[n]), (name, n, v)
            else:
                assert v is (buffers[n] if n in buffers else getattr(tk, n)), (name, n, v)         # the very buffer: identity
    got = dict(zip(track.ENTRY_ARGS[entry], tk._plan[0][1]))
    if gate is not None:                                           # gate_d2 directly behind velocity_var, pred_d2 last
        at = track.ENTRY_ARGS[entry].index("velocity_var")
        assert tk._plan[0][1][at:at + 2] == (4e-2, 9.5) and tk._plan[0][1][-1] is tk.pred_d2 and tk._plan[0][1][-2] is tk.pred_boxes
    else:
        assert "gate_d2" not in got and "pred_d2" not in got
    assert ("where" in got) == ("pred_where" in got) == bool(motion)
