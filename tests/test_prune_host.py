"""Host-side tests of subset pruning (attend_infer_repeat_amd/prune.py): the argument checks, `reference_select` -- the numpy float64
restatement of air_prune_select -- against a literal brute force and on crafted tables of joints, the stable partition, the evidence on
a hand case, `reference_score` on a 3x3 / 2x2 case worked by hand, and the new entries in the header and the binding.  No GPU."""
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from attend_infer_repeat_amd import prune
from attend_infer_repeat_amd.engine_config import EngineConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "air_hip.h")
HL2PI = 0.5 * math.log(2 * math.pi)


# ---- 1. check_arguments ---------------------------------------------------------------------------------------------------------
def test_check_arguments_accepts_the_scripts_configuration():
    cfg = EngineConfig(max_steps=3, explore_eps=1e-3, steps_pred_hidden=(128, 64), transform_var_bias=.5, step_bias=.75,
                       output_multiplier=.5)
    prune.check_arguments(cfg)
    prune.check_arguments(cfg, "all")
    prune.check_arguments(dataclasses.replace(cfg, max_steps=6, where_shift_prior=(None, 1.0)), "present")
    prune.check_arguments(dataclasses.replace(cfg, mfma_dtype="bf16"), "all")         # nothing here runs the decoder


@pytest.mark.parametrize("change,cand,match", [
    (dict(max_steps=7), "present", "64 subsets"), (dict(max_steps=32), "all", "64 subsets"),
    (dict(), "absent", "candidates"), (dict(), None, "candidates"),
    (dict(discrete_steps=False), "present", "discrete_steps"), (dict(what_prior=None), "present", "what_prior"),
    (dict(where_scale_prior=None), "all", "where_scale_prior"), (dict(where_shift_prior=None), "all", "where_shift_prior")])
def test_check_arguments_refuses(change, cand, match):
    with pytest.raises(ValueError, match=match):
        prune.check_arguments(dataclasses.replace(EngineConfig(), **change), cand)


# ---- 2. reference_select ----------------------------------------------------------------------------------------------------------
def select_case(T, B, A, G, seed, n=None):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s)
    if n is None:
        n = rng.integers(0, T + 1, B)
        n[0] = T
        if B > 1:
            n[1] = 0
    presence = (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(np.float64)
    return dict(what=r(T, B, A), where=r(T, B, 4), glimpse=r(T, B, G), score=rng.uniform(size=(T, B)), presence=presence,
                where_loc=r(T, B, 4), rec_sub=np.abs(r(2, B, 1 << T)) * 20)


def brute_force(case, priors, prior, normalize, all_candidates):
    """every mask's J from the formula, written out per image and per mask; the best by the visiting order"""
    T, B, A = case["what"].shape
    n = [int(np.cumprod(case["presence"][:, b] > 0.5).sum()) for b in range(B)]
    logn = lambda x, mu, sd: -0.5 * ((x - mu) / sd) ** 2 - math.log(sd) - HL2PI
    tot = sum(prior) if normalize else 1.0
    J = np.full((B, 1 << T), np.nan)
    best = []
    for b in range(B):
        c = T if all_candidates else n[b]
        for m in range(1 << c):
            v = -(case["rec_sub"][0, b, m] + case["rec_sub"][1, b, m])
            lat = 0.0
            for t in range(T):
                if (m >> t) & 1:
                    lp = sum(logn(x, priors[0], priors[1]) for x in case["what"][t, b])
                    for j in range(4):
                        if j % 2 == 0:
                            lp += logn(case["where"][t, b, j], priors[2], priors[3])
                        else:
                            mu = case["where_loc"][t, b, j] if priors[4] is None else priors[4]
                            lp += logn(case["where"][t, b, j], mu, priors[5])
                    lat += lp
            J[b, m] = v + lat + math.log(prior[bin(m).count("1")] / tot)
        m0 = (1 << n[b]) - 1
        order = [m0] + [m for m in range((1 << c) - 1, -1, -1) if m != m0]
        bm = order[0]
        for m in order[1:]:
            if J[b, m] > J[b, bm]:
                bm = m
        best.append(bm)
    return J, np.array(best), np.array(n)


@pytest.mark.parametrize("all_candidates", [False, True])
@pytest.mark.parametrize("shift_loc", [0.25, None])
@pytest.mark.parametrize("T", [1, 3, 6])
def test_reference_select_matches_brute_force(T, shift_loc, all_candidates):
    B, A, G = 5, 3, 4
    case = select_case(T, B, A, G, seed=T)
    priors = (0.1, 1.5, 1.0, 0.5, shift_loc, 2.0)
    prior = np.random.default_rng(9).uniform(0.1, 1.0, T + 1)
    for normalize in (False, True):
        ref = prune.reference_select(**case, priors=priors, prior=prior, normalize_prior=normalize, all_candidates=all_candidates)
        J, best, n = brute_force(case, priors, prior, normalize, all_candidates)
        assert np.allclose(ref["J_sub"], J, rtol=1e-12, atol=1e-9, equal_nan=True)
        assert np.array_equal(ref["best_mask"], best) and np.array_equal(ref["n"], n)
        assert np.array_equal(ref["num_objects"], [bin(int(m)).count("1") for m in best])
        rows = np.arange(B)
        assert np.array_equal(ref["objective"], ref["J_sub"][rows, best])
        assert np.array_equal(ref["objective_start"], ref["J_sub"][rows, (1 << n) - 1])
        assert (ref["objective"] >= ref["objective_start"]).all()
        if not all_candidates:                                     # "present" can only remove: no bit at or above n
            assert ((best >> n) == 0).all()
            assert np.isnan(ref["J_sub"][0, :]).sum() == 0 and np.isnan(ref["J_sub"][1, 1:]).all()      # n = T resp. n = 0
        # the compacted rows are the source rows of kept_step
        for b in range(B):
            ks = ref["kept_step"][:, b]
            assert list(ks) == prune.partition(int(best[b]), T) and sorted(ks) == list(range(T))
            for k in ("what", "where", "glimpse", "score"):
                assert np.array_equal(ref[k][:, b], case[k][ks, b]), k


def crafted(J_rows, n, T, all_candidates=True):
    return prune.select_masks(np.array(J_rows, np.float64), np.array(n), T, all_candidates)


def test_visiting_order_and_tie_rule():
    nan, inf = float("nan"), float("inf")
    # T = 2, masks 0..3; n = 1: m0 = 1; visiting order with all candidates: 1, then 3, 2, 0
    assert crafted([[5.0, 5.0, 5.0, 5.0]], [1], 2).tolist() == [1]             # equal J keeps m0
    assert crafted([[5.0, 4.0, 5.0, 5.0]], [1], 2).tolist() == [3]             # among equals the first visited: from the full mask down
    assert crafted([[6.0, 4.0, 5.0, nan]], [1], 2).tolist() == [0]             # a NaN never wins
    assert crafted([[nan, 4.0, nan, nan]], [1], 2).tolist() == [1]
    assert crafted([[nan, nan, nan, nan]], [1], 2).tolist() == [1]             # all-NaN keeps m0
    assert crafted([[nan, nan, 2.0, nan]], [1], 2).tolist() == [2]             # a NaN start is replaced by the first number
    assert crafted([[-inf, -inf, -7.0, -inf]], [1], 2).tolist() == [2]         # -inf loses to anything finite
    assert crafted([[-inf, -inf, -inf, -inf]], [1], 2).tolist() == [1]         # ... and ties with itself
    assert crafted([[nan, -inf, nan, nan]], [1], 2).tolist() == [1]
    assert crafted([[nan, nan, nan, -inf]], [1], 2).tolist() == [3]            # -inf is an ordinary value: it replaces a NaN
    # "present": masks at or above 2^n are never visited, whatever the table holds there
    assert crafted([[1.0, 2.0, 99.0, 99.0]], [1], 2, all_candidates=False).tolist() == [1]
    assert crafted([[3.0, 2.0, 99.0, 99.0]], [1], 2, all_candidates=False).tolist() == [0]
    assert crafted([[3.0, 99.0, 99.0, 99.0]], [0], 2, all_candidates=False).tolist() == [0]


def test_stable_partition():
    assert prune.partition(0b000, 3) == [0, 1, 2]
    assert prune.partition(0b111, 3) == [0, 1, 2]
    assert prune.partition(0b101, 3) == [0, 2, 1]
    assert prune.partition(0b010, 3) == [1, 0, 2]
    assert prune.partition(0b101000, 6) == [3, 5, 0, 1, 2, 4]
    assert prune.partition(0b1, 1) == [0]


def test_evidence_signs_on_a_hand_case():
    """T = 2, n = 2, A = 1, all latents at their prior means with unit scales: lp_t = -5/2 log 2 pi; a flat count prior.  Step 0
    explains 10 nats of the image, step 1 costs 1 nat of it."""
    z = lambda *s: np.zeros(s)
    rec = np.array([[[20.0, 10.0, 21.0, 11.0]]])                    # masks: none, {0}, {1}, {0, 1}
    ref = prune.reference_select(z(2, 1, 1), z(2, 1, 4), z(2, 1, 2), z(2, 1), np.ones((2, 1)), None, (0, 1, 0, 1, 0, 1),
                                 np.ones(3), True, False, rec)
    lp = -5 * HL2PI
    assert np.allclose(ref["lp"], lp)
    assert np.allclose(ref["J_sub"][0], [-20 - math.log(3), -10 + lp - math.log(3), -21 + lp - math.log(3), -11 + 2 * lp - math.log(3)])
    assert np.allclose(ref["evidence"][:, 0], [10 + lp, -1 + lp])   # J({0,1}) - J({1}),  J({0,1}) - J({0})
    assert ref["evidence"][0, 0] > 0 > ref["evidence"][1, 0]
    assert ref["best_mask"].tolist() == [1] and ref["kept_step"][:, 0].tolist() == [0, 1] and ref["num_objects"].tolist() == [1]
    # n = 1 and "present": step 1 is no candidate, its evidence is NaN; with "all" it is J({0,1}) - J({0})
    pres = np.array([[1.0], [0.0]])
    a = prune.reference_select(z(2, 1, 1), z(2, 1, 4), z(2, 1, 2), z(2, 1), pres, None, (0, 1, 0, 1, 0, 1), np.ones(3), True, False, rec)
    assert np.isclose(a["evidence"][0, 0], 10 + lp) and math.isnan(a["evidence"][1, 0]) and np.isnan(a["J_sub"][0, 2:]).all()
    b = prune.reference_select(z(2, 1, 1), z(2, 1, 4), z(2, 1, 2), z(2, 1), pres, None, (0, 1, 0, 1, 0, 1), np.ones(3), True, True, rec)
    assert np.allclose(b["evidence"][:, 0], [10 + lp, -1 + lp]) and b["best_mask"].tolist() == [1]


def test_the_count_prior_enters():
    """two masks that differ only in log pi: a prior that favours one object flips the decision"""
    z = lambda *s: np.zeros(s)
    rec = np.array([[[10.0, 10.0 - 5 * HL2PI]]])                    # T = 1: J(0) = -10 + log pi(0), J(1) = -10 + log pi(1)
    args = (z(1, 1, 1), z(1, 1, 4), z(1, 1, 2), z(1, 1), np.ones((1, 1)), None, (0, 1, 0, 1, 0, 1))
    assert prune.reference_select(*args, np.array([0.3, 0.7]), True, False, rec)["best_mask"].tolist() == [1]
    assert prune.reference_select(*args, np.array([0.7, 0.3]), True, False, rec)["best_mask"].tolist() == [0]
    un = prune.reference_select(*args, np.array([0.7, 0.3]), False, False, rec)
    no = prune.reference_select(*args, np.array([1.4, 0.6]), True, False, rec)
    assert np.allclose(un["J_sub"], no["J_sub"])


# ---- 3. reference_score by hand -------------------------------------------------------------------------------------------------------
def test_reference_score_on_a_3x3_canvas_by_hand():
    """where = (1, 0, 1, 0): the 2x2 glimpse is stretched over the 3x3 canvas, pixel coordinates 0, 1/2, 1 on both axes.
    glimpse_0 = [[1, 0], [0, 0]] -> layer_0 = [[1, .5, 0], [.5, .25, 0], [0, 0, 0]];  glimpse_1 = [[0, 0], [0, 2]] ->
    layer_1 = [[0, 0, 0], [0, .5, 1], [0, 1, 2]];  obs = layer_0, mult = std = 1."""
    glimpse = np.array([[[[1.0, 0.0], [0.0, 0.0]]], [[[0.0, 0.0], [0.0, 2.0]]]])
    where = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1, 1))
    l0 = np.array([[1, .5, 0], [.5, .25, 0], [0, 0, 0]])
    l1 = np.array([[0, 0, 0], [0, .5, 1], [0, 1, 2]])
    assert np.allclose(prune._st_write(glimpse[0], where[0], (3, 3))[0], l0, atol=1e-15)
    assert np.allclose(prune._st_write(glimpse[1], where[1], (3, 3))[0], l1, atol=1e-15)
    got = prune.reference_score(glimpse, where, np.ones((2, 1)), l0[None], 1.0, 1.0, False)
    assert np.allclose(got[0], np.array([0.78125, 0.0, 3.78125, 3.125]) + 9 * HL2PI, atol=1e-12)
    # mult and std: obs = 2 * layer_0 is explained exactly by mask 1 under mult = 2; std = 2 quarters the squares and adds 9 log 2
    got = prune.reference_score(glimpse, where, np.ones((2, 1)), 2 * l0[None], 2.0, 2.0, False)
    assert np.allclose(got[0], np.array([0.78125, 0.0, 3.78125, 3.125]) + 9 * (HL2PI + math.log(2.0)), atol=1e-12)
    # n = 1: "present" leaves masks 2, 3 unwritten; "all" scores them
    pres = np.array([[1.0], [0.0]])
    assert np.isnan(prune.reference_score(glimpse, where, pres, l0[None], 1.0, 1.0, False)[0, 2:]).all()
    assert np.allclose(prune.reference_score(glimpse, where, pres, l0[None], 1.0, 1.0, True)[0, 2:], np.array([3.78125, 3.125]) + 9 * HL2PI)
    # a glimpse shifted wholly off the canvas contributes nothing; a flipped one mirrors
    far = where.copy()
    far[1, 0] = [1.0, 5.0, 1.0, 0.0]
    assert (prune._st_write(glimpse[1], far[1], (3, 3)) == 0).all()
    flip = np.array([[-1.0, 0.0, 1.0, 0.0]])
    assert np.allclose(prune._st_write(glimpse[0], flip, (3, 3))[0], l0[:, ::-1], atol=1e-15)


# ---- 4. the entries -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_on_the_engine_side_and_bound():
    from attend_infer_repeat_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("air_prune_score", 16), ("air_prune_select", 33), ("air_prune_relabel", 10)):
        m = re.search(r"AIR_ENGINE_API\s+int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert "prune_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "prune_kernels.hip"))
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5


def test_argument_checks_need_no_device():
    """NULL / bad-shape arguments return AIR_E_* before any launch"""
    from attend_infer_repeat_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert lib.air_prune_score(None, None, None, None, 1.0, 1.0, 0, 3, 1, 8, 8, 4, 4, 1, None, None) == -1
    assert lib.air_prune_select(*([None] * 6), 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, None, 1, 0, None, 1, 3, 1, 4, 4, *([None] * 12)) == -1
    assert lib.air_prune_relabel(None, None, None, None, 3, 1, None, None, None, None) == -1
    import ctypes
    buf = (ctypes.c_double * 64)()                                  # any non-NULL, 16-byte aligned host address: never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    for T in (0, 7, 32):
        assert lib.air_prune_score(p, p, p, p, 1.0, 1.0, 0, T, 1, 8, 8, 4, 4, 8, p, None) == -2
        assert lib.air_prune_relabel(p, p, p, p, T, 1, p, p, p, None) == -2
    assert lib.air_prune_score(p, p, p, p, 1.0, 1.0, 0, 3, 1, 8, 8, 4, 4, 3, p, None) == -2       # not the library's banding
