"""Host-side tests of the temporal proposals (attend_infer_repeat_amd/temporal.py): the argument checks, `reference_pool` -- the numpy
float64 restatement of air_temporal_pool -- on hand-built rows, the filler rows under prune.reference_select, the planted sequence
through reference_pool -> prune.reference_score -> prune.reference_select, and the new entry in the header and the binding.  No GPU."""
import dataclasses
import os
import re

import numpy as np
import pytest

from temporal_cases import MULT, OUT_TOL, PLANTED, PRIORS, STD, chain, planted_reference, planted_sequence, pool_rows

from attend_infer_repeat_amd import prune, temporal
from attend_infer_repeat_amd.engine_config import EngineConfig
from attend_infer_repeat_amd.temporal import ABSENT, DUPLICATE, FULL, KNOWN, NONFINITE, TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "air_hip.h")
CFG = EngineConfig(max_steps=3, explore_eps=1e-3, steps_pred_hidden=(128, 64), transform_var_bias=.5, step_bias=.75, output_multiplier=.5)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. check_arguments ---------------------------------------------------------------------------------------------------------
def test_check_arguments_accepts_the_scripts_configuration():
    assert temporal.check_arguments(CFG, 8, 1024, 1, 1, 0.3) == (3, 8, 128)
    assert temporal.check_arguments(CFG, 8) == (3, 8, None)
    assert temporal.check_arguments(CFG, 1, 5, 3, 2, 0.0) == (3, 1, 5)
    assert [temporal.max_proposals(T) for T in range(1, 7)] == [2, 4, 3, 2, 1, 0]
    for T in range(1, 6):
        temporal.check_arguments(dataclasses.replace(CFG, max_steps=T), 2, 4, temporal.max_proposals(T))


@pytest.mark.parametrize("change,args,match", [
    (dict(), (8, 1024, 4), "proposals"), (dict(max_steps=1), (8, 1024, 3), "proposals"), (dict(max_steps=5), (8, 1024, 2), "proposals"),
    (dict(max_steps=6), (8, 1024, 1), "proposals"), (dict(), (8, 1024, 0), "proposals"), (dict(), (8, 1024, True), "proposals"),
    (dict(), (8, 1024, 1, 0), "rounds"), (dict(), (8, 1024, 1, -1), "rounds"), (dict(), (8, 1024, 1, 1.5), "rounds"),
    (dict(), (8, 1020, 1), "multiple"), (dict(), (3, 1024), "multiple"), (dict(), (0, 1024), "n_frames"),
    (dict(), (8, 1024, 1, 1, 1.5), "iou_novel"), (dict(), (8, 1024, 1, 1, float("nan")), "iou_novel"),
    (dict(where_shift_prior=(None, 1.0)), (8, 1024), "loc"), (dict(max_steps=7), (8, 1024), "64 subsets"),
    (dict(what_prior=None), (8, 1024), "what_prior")])
def test_check_arguments_refuses(change, args, match):
    with pytest.raises(ValueError, match=match):
        temporal.check_arguments(dataclasses.replace(CFG, **change), *args)


# ---- 2. reference_pool on hand-built rows ---------------------------------------------------------------------------------------------
IMG = (20, 20)
HERE, THERE, FAR = (0.3, -0.5, 0.3, -0.5), (0.3, 0.5, 0.3, 0.5), (0.3, 0.5, 0.3, -0.5)


def rows(T, F, places, n, score=None, A=3, G=4, S=1):
    """places[f] = the where rows of frame f's slots (short lists are padded with a row far outside)"""
    R = S * F
    rng = np.random.default_rng(1)
    where = np.empty((T, R, 4), np.float32)
    where[:] = (0.1, 3.0, 0.1, 3.0)
    for r, rows_ in enumerate(places):
        for t, wr in enumerate(rows_):
            where[t, r] = wr
    return dict(what=rng.normal(size=(T, R, A)).astype(np.float32), where=where, glimpse=rng.normal(size=(T, R, G)).astype(np.float32),
                score=np.full((T, R), 0.5, np.float32) if score is None else np.asarray(score, np.float32), n=np.asarray(n),
                prior=np.linspace(0.2, 0.4, T + 1))


def pool_of(case, F, P=1, **kw):
    return temporal.reference_pool(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["prior"], F, IMG, P, **kw)


def is_filler(pool, j, r):
    return (np.isnan(pool["what"][j, r]).all() and bits(pool["what"][j, r]).tolist() == [0x7fc00000] * pool["what"].shape[2]
            and pool["where"][j, r].tolist() == [1, 0, 1, 0] and not pool["glimpse"][j, r].any() and pool["score"][j, r] == 0
            and pool["source"][j, r] == -1)


def test_one_frame_gives_only_filler_rows():
    T, P, R = 2, 2, 3
    case = rows(T, 1, [[HERE, THERE]] * R, [2, 1, 0], S=R)
    pool = pool_of(case, 1, P)
    assert (pool["cand_state"] == ABSENT).all() and (pool["taken"] == 0).all() and (pool["partner"] == -1).all()
    for k in ("what", "where", "glimpse", "score"):
        assert np.array_equal(bits(pool[k][:T]), bits(case[k])), k  # the current rows, bit for bit
    assert all(is_filler(pool, j, r) for j in (T, T + 1) for r in range(R))
    assert np.array_equal(pool["presence"], chain([2, 1, 0], T + P)) and np.array_equal(pool["source"][:T], [[0] * R, [1] * R])
    assert np.array_equal(pool["prior"], list(case["prior"]) + [0.0] * P)


def test_first_and_last_frame_see_one_side_and_sequences_do_not_mix():
    T, F, S = 1, 3, 2
    case = rows(T, F, [[HERE], [THERE], [FAR]] * S, [1] * (S * F), S=S)
    pool = pool_of(case, F, 1)
    for s in range(S):
        first, mid, last = (s * F + f for f in range(F))
        assert pool["cand_state"][first].tolist() == [ABSENT, TAKEN] and pool["cand_state"][last].tolist() == [TAKEN, ABSENT]
        assert pool["cand_state"][mid].tolist() == [TAKEN, FULL]   # equal scores: the lower q, the past side
        assert np.array_equal(bits(pool["where"][1, first]), bits(case["where"][0, mid]))
        assert np.array_equal(bits(pool["where"][1, last]), bits(case["where"][0, mid]))
        assert np.array_equal(bits(pool["what"][1, mid]), bits(case["what"][0, first]))
        assert pool["source"][1, first] == T + 1 and pool["source"][1, last] == T + 0
    past = pool_of(case, F, 1, both_sides=False)
    assert past["cand_state"][:, 1].tolist() == [ABSENT] * (S * F) and past["taken"].tolist() == [0, 1, 1] * S
    assert is_filler(past, 1, 0) and past["cand_state"][1].tolist() == [TAKEN, ABSENT]


def test_equal_scores_take_the_lower_q_and_unequal_ones_the_higher_score():
    T, F = 2, 3
    places = [[THERE, FAR], [HERE], [(0.3, -0.5, 0.3, 0.5), (0.3, 0.0, 0.3, 0.0)]]
    case = rows(T, F, places, [2, 1, 2])
    pool = pool_of(case, F, 2)
    assert pool["cand_state"][1].tolist() == [TAKEN, TAKEN, FULL, FULL] and pool["source"][2:, 1].tolist() == [T + 0, T + 1]
    case["score"][1, 2] = 0.75                                     # q = 3 now leads; q = 0 is second
    pool = pool_of(case, F, 2, round=2)
    assert pool["cand_state"][1].tolist() == [TAKEN, FULL, FULL, TAKEN] and pool["source"][2:, 1].tolist() == [T + 8 + 3, T + 8 + 0]
    assert np.array_equal(bits(pool["glimpse"][2, 1]), bits(case["glimpse"][1, 2])) and pool["score"][2, 1] == np.float32(0.75)


def test_a_nan_what_candidate_is_nonfinite():
    T, F = 1, 2
    for key, idx, bad in (("what", (0, 0, 2), np.nan), ("where", (0, 0, 1), np.inf), ("score", (0, 0), -np.inf)):
        case = rows(T, F, [[THERE], [HERE]], [1, 1])
        case[key][idx] = bad
        pool = pool_of(case, F, 1)
        assert pool["cand_state"][1].tolist() == [NONFINITE, ABSENT] and pool["taken"][1] == 0 and is_filler(pool, 1, 1), key
    case = rows(T, F, [[THERE], [HERE]], [1, 1])
    case["glimpse"][0, 0, 1] = np.nan                              # the glimpse is not checked: the NaN travels into the pool
    pool = pool_of(case, F, 1)
    assert pool["cand_state"][1].tolist() == [TAKEN, ABSENT] and np.isnan(pool["glimpse"][1, 1, 1])


@pytest.mark.parametrize("interpolate", [True, False])
def test_an_object_in_both_neighbours_is_one_taken_and_one_duplicate(interpolate):
    T, F = 2, 3
    a, c = (0.3, 0.45, 0.31, 0.5), (0.32, 0.55, 0.3, 0.52)
    case = rows(T, F, [[HERE, a], [HERE], [c, HERE]], [2, 1, 2], score=[[0.9, 0.9, 0.6], [0.4, 0.1, 0.9]])
    pool = pool_of(case, F, 2, interpolate=interpolate)
    # q = 0, 3: HERE is known; q = 2 (score 0.6) leads q = 1 (0.4): taken from the NEXT frame, its partner the past sighting
    assert pool["cand_state"][1].tolist() == [KNOWN, DUPLICATE, TAKEN, KNOWN] and pool["taken"][1] == 1
    assert pool["partner"][:, 1].tolist() == [1, -1] and is_filler(pool, 3, 1)
    mid = (0.5 * (np.float32(c).astype(np.float64) + np.float32(a).astype(np.float64))).astype(np.float32)
    assert np.array_equal(bits(pool["where"][2, 1]), bits(mid if interpolate else np.float32(c)))
    for k in ("what", "glimpse", "score"):
        assert np.array_equal(bits(pool[k][2, 1]), bits(case[k][0, 2])), k      # always the taken one's bits
    assert pool["source"][2, 1] == T + 2
    # a duplicate of the SAME side is no partner
    case = rows(T, F, [[a, c], [HERE], [FAR]], [2, 1, 1], score=[[0.9, 0.9, 0.2], [0.4, 0.1, 0.9]])
    pool = pool_of(case, F, 2, interpolate=interpolate)
    assert pool["cand_state"][1].tolist() == [TAKEN, DUPLICATE, TAKEN, ABSENT] and pool["partner"][:, 1].tolist() == [-1, -1]
    assert np.array_equal(bits(pool["where"][2, 1]), bits(np.float32(a)))


def test_full_occurs_when_more_than_P_candidates_are_novel():
    T, F = 3, 2
    case = rows(T, F, [[HERE, THERE, FAR], []], [3, 0], score=[[0.3, 0.5], [0.9, 0.5], [0.6, 0.5]])
    pool = pool_of(case, F, 2)
    assert pool["cand_state"][1].tolist() == [FULL, TAKEN, TAKEN, ABSENT, ABSENT, ABSENT] and pool["taken"][1] == 2
    assert pool["source"][3:, 1].tolist() == [T + 1, T + 2] and pool["presence"][:, 1].tolist() == [0] * 5


def test_known_is_strictly_above_iou_novel():
    """two 8 x 8 boxes on a 16-pixel canvas, shifted by 4 pixels along x: IoU = 32 / 96 = 1 / 3 exactly in float64"""
    T, F = 1, 2
    case = rows(T, F, [[(0.5, 0.0, 0.5, 0.0)], [(0.5, 0.5, 0.5, 0.0)]], [1, 1])
    kw = dict(what=case["what"], where=case["where"], glimpse=case["glimpse"], score=case["score"], n=case["n"], prior=case["prior"],
              n_frames=F, img_size=(16, 16), proposals=1)
    boxes = temporal.reference_pool(**kw)["boxes"]
    assert boxes[0, 0].tolist() == [4, 4, 8, 8] and boxes[0, 1].tolist() == [8, 4, 8, 8]
    third = temporal.box_iou(boxes[0, 0], boxes[0, 1])
    assert third == 32.0 / 96.0
    assert temporal.reference_pool(**kw, iou_novel=third)["cand_state"][1].tolist() == [TAKEN, ABSENT]      # at the bar: not known
    assert temporal.reference_pool(**kw, iou_novel=np.nextafter(third, 0.0))["cand_state"][1].tolist() == [KNOWN, ABSENT]
    assert temporal.reference_pool(**kw, iou_novel=third - 1e-3)["cand_state"][1].tolist() == [KNOWN, ABSENT]


def test_random_rows_keep_the_pool_invariants():
    seen = set()
    for T, P, S, F in ((2, 4, 2, 5), (3, 3, 2, 3), (5, 1, 3, 2), (1, 2, 2, 5)):
        case = pool_rows(T, S, F, 3, 4, seed=T * 7 + F)
        for both in (True, False):
            pool = temporal.reference_pool(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["prior"], F,
                                           (24, 24), P, 0.3, both, True, round=1)
            st = pool["cand_state"]
            assert np.array_equal((st == TAKEN).sum(1), pool["taken"]) and (pool["taken"] <= P).all()
            assert ((st == FULL).sum(1) == 0)[pool["taken"] < P].all()           # FULL only once P are taken
            for r in range(S * F):
                src = pool["source"][T:, r]
                assert (src[:pool["taken"][r]] >= T + 2 * T).all() and (src[pool["taken"][r]:] == -1).all()
                assert st[r, src[:pool["taken"][r]] - 3 * T].tolist() == [TAKEN] * pool["taken"][r]
                if r % F == 0:
                    assert (st[r, :T] == ABSENT).all()
                if r % F == F - 1 or not both:
                    assert (st[r, T:] == ABSENT).all()
            seen |= set(st.reshape(-1).tolist())
    assert seen == {ABSENT, TAKEN, KNOWN, DUPLICATE, FULL, NONFINITE}       # the cases the GPU test runs reach every state


# ---- 3. filler rows under the selection ---------------------------------------------------------------------------------------------
def test_a_filler_row_is_never_selected():
    T, F, P = 2, 1, 1
    case = rows(T, F, [[HERE, THERE]] * 3, [2, 1, 0], S=3)
    pool = pool_of(case, F, P)
    C, B = T + P, 3
    rec = np.full((B, 1 << C), 1e6)                                # every mask without the filler is bad ...
    rec[:, 4:] = 0.0                                               # ... every mask with it would be perfect
    sel = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, PRIORS,
                                 pool["prior"], 1, 1, rec)
    assert np.isnan(sel["J_sub"][:, 4:]).all() and np.isfinite(sel["J_sub"][:, :4]).all()
    assert ((sel["best_mask"] >> T) == 0).all() and np.isnan(sel["evidence"][T]).all()
    # a table whose masks without the filler are ALL worse than a (hypothetical) finite joint of a mask with it: select_masks on the
    # NaN table still never takes one
    J = np.where(np.isnan(sel["J_sub"]), np.nan, -1e30)
    assert ((prune.select_masks(J, sel["n"], C, True) >> T) == 0).all()


# ---- 4. the planted sequence ----------------------------------------------------------------------------------------------------------------
def check_frames_0_and_2_keep_their_parse(case, pool, sel):
    T = PLANTED["T"]
    for r in (0, 2):
        assert pool["taken"][r] == 0 and set(pool["cand_state"][r].tolist()) <= {ABSENT, KNOWN}
        assert sel["best_mask"][r] == 3 and sel["num_objects"][r] == 2 and sel["kept_step"][:, r].tolist() == [0, 1, 2]
        assert sel["objective"][r] == sel["objective_start"][r]
        for k in ("what", "where", "glimpse", "score"):
            assert np.array_equal(bits(sel[k][:T, r]), bits(case[k][:, r])), k


@pytest.mark.parametrize("motion", [True, False])
def test_planted_sequence_recovers_the_missed_object(motion):
    """interpolate=True with motion, and interpolate=False without: frame 1 ends with two objects, the second one the candidate"""
    T = PLANTED["T"]
    case = planted_sequence(motion)
    pool, rec, sel = planted_reference(case, interpolate=motion)
    assert pool["cand_state"][1].tolist() == [KNOWN, TAKEN, KNOWN, DUPLICATE] and pool["partner"][0, 1] == 3
    if motion:                                                     # the midpoint of the two sightings is the object's place in frame 1
        assert np.abs(pool["where"][2, 1].astype(np.float64) - case["truth"][1]).max() < 1e-7
    else:
        assert np.array_equal(bits(pool["where"][2, 1]), bits(case["truth"][0]))
    assert sel["best_mask"][1] == 0b101 and sel["num_objects"][1] == 2 and sel["kept_step"][:, 1].tolist() == [0, 2, 1]
    assert sel["source_out"][:, 1].tolist() == [0, T + 1, 1]       # kept_step - T = round * 2T + q = 1: slot 1 of frame 0
    assert sel["objective"][1] > sel["objective_start"][1]
    J = sel["J_sub"][1]
    order = np.sort(J[np.isfinite(J)])[::-1]
    lead, bar = order[0] - order[1], 2 * OUT_TOL * np.abs(sel["J_sub"][np.isfinite(sel["J_sub"])]).max()
    print("planted (motion=%s): J start %.4f -> %.4f, lead %.4f, bar %.4g" % (motion, sel["objective_start"][1], order[0], lead, bar))
    assert lead > bar                                              # the GPU version of the case can compare decisions exactly
    assert sel["num_objects"].tolist() == [2, 2, 2] and (sel["num_objects"] <= T).all()
    check_frames_0_and_2_keep_their_parse(case, pool, sel)


def test_planted_sequence_with_motion_and_no_interpolation_is_never_worse():
    case = planted_sequence(True)
    pool, rec, sel = planted_reference(case, interpolate=False)
    assert np.array_equal(bits(pool["where"][2, 1]), bits(case["truth"][0]))      # the past sighting's own place
    assert (sel["objective"] >= sel["objective_start"]).all()
    check_frames_0_and_2_keep_their_parse(case, pool, sel)


def test_planted_sequence_from_the_past_only():
    case = planted_sequence(True)
    pool, rec, sel = planted_reference(case, interpolate=True, both_sides=False)
    assert pool["cand_state"][1].tolist() == [KNOWN, TAKEN, ABSENT, ABSENT] and pool["partner"][0, 1] == -1
    assert np.array_equal(bits(pool["where"][2, 1]), bits(case["truth"][0])) and (sel["objective"] >= sel["objective_start"]).all()


# ---- 5. the header and the binding ------------------------------------------------------------------------------------------------------
def test_the_new_entry_is_declared_bound_and_built():
    from attend_infer_repeat_amd import _lib, build
    text = open(HEADER).read()
    m = re.search(r"AIR_ENGINE_API int air_temporal_pool\(([^;]*)\);", text)
    assert m, "air_temporal_pool is not declared AIR_ENGINE_API"
    params = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["air_temporal_pool"]
    assert len(params) == len(args) == 31 and params[-1] == "void *stream"
    assert [("*" in a) for a in params] == [a is _lib.P for a in args]
    assert args[17] is __import__("ctypes").c_double and params[17] == "double iou_novel"
    assert "temporal_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "temporal_kernels.hip"))
    assert re.search(r"#define AIR_ABI_VERSION 10\b", text) and re.search(r"#define AIR_ENGINE_ABI_VERSION 5\b", text)
