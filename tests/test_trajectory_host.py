"""Host-side tests of the trajectory smoother (attend_infer_repeat_amd/trajectory.py): `reference_smooth` -- the numpy float64 restatement
of air_track_smooth -- against an independent matrix-form smoother, its exact invariants, the completed and the forecast table, the
argument checks, and the identity figures of the planted linear sequences.  No GPU.

Bars.  reference_smooth and the matrix form are two float64 codings of one recursion on values of magnitude <= 1: 1e-12 absolute
(the difference seen is of order 1e-16; this is no device tolerance).  Everything else is exact: integers, or bits."""
import os
import re

import numpy as np
import pytest

from trajectory_cases import (IMG, PLANTED, drifting_case, full_table_case, jumping_case, matrix_smoother, planted_sequences,
                              planted_where, reference, rows_from_objects, with_tracker)

from attend_infer_repeat_amd import track, trajectory
from attend_infer_repeat_amd.tile import scene_boxes
from attend_infer_repeat_amd.trajectory import ABSENT, FILLED, FORECAST, OBSERVED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_check_arguments():
    assert trajectory.check_arguments(3, 8, 1024, 1, 4) == (3, 8, 128, 6, 4, (1e-4, 1e-4), 4e-4, 0.04)
    assert trajectory.check_arguments(3, 8, None, 0)[2:4] == (None, 3)
    assert [trajectory.completed_rows(T, a) for T, a in ((3, 0), (3, 1), (3, 2), (32, 1), (6, 9))] == [3, 6, 9, 32, 32]
    nan = float("nan")
    for kw, word in ((dict(process_noise=(0.0, 1e-4)), "process_noise"), (dict(process_noise=(1e-4, -1.0)), "process_noise"),
                     (dict(process_noise=(nan, 1e-4)), "process_noise"), (dict(process_noise=1e-4), "process_noise"),
                     (dict(measurement_noise=0.0), "measurement_noise"), (dict(measurement_noise=nan), "measurement_noise"),
                     (dict(velocity_var=-1e-9), "velocity_var"), (dict(velocity_var=nan), "velocity_var"), (dict(horizon=17), "horizon"),
                     (dict(horizon=-1), "horizon"), (dict(horizon=1.5), "horizon"), (dict(max_age=-1), "max_age"),
                     # outside the supported noise domain: the rule loses the posterior mean there
                     (dict(velocity_var=1e6), "V_OVER_R_MAX"), (dict(velocity_var=401.0), "V_OVER_R_MAX"),
                     (dict(process_noise=(1.0, 1.0), measurement_noise=3e-17, velocity_var=0.0), "Q_OVER_R_MAX"),
                     (dict(process_noise=(1e-4, 1e-33)), "Q_OVER_R_MIN"), (dict(process_noise=(4.1e11, 1e-4)), "Q_OVER_R_MAX"),
                     (dict(process_noise=(1e-300,) * 2, measurement_noise=1e-300, velocity_var=0.0), "R_MIN"),
                     (dict(process_noise=(1e140,) * 2, measurement_noise=1e140), "R_MAX")):
        with pytest.raises(ValueError, match=word):
            trajectory.check_arguments(3, 8, 16, **kw)
    with pytest.raises(ValueError, match="max_steps"):
        trajectory.check_arguments(33, 8, 16)
    with pytest.raises(ValueError, match="int16"):
        trajectory.check_arguments(32, 1024, 1024)
    with pytest.raises(ValueError, match="multiple"):
        trajectory.check_arguments(3, 8, 15)
    assert trajectory.check_arguments(3, 8, 16, velocity_var=0.0)[-1] == 0.0
    assert trajectory.check_arguments(3, 8, 16, velocity_var=400.0)[-1] == 400.0      # velocity_var / measurement_noise = 1e6: the limit


@pytest.mark.parametrize("max_age,seed", [(1, 0), (2, 1), (0, 2), (3, 3)])
def test_reference_is_the_matrix_form(max_age, seed):
    case = drifting_case(3, 8, 3, max_age, seed=seed)
    noise = dict(process_noise=(3e-4, 1e-4), measurement_noise=5e-4, velocity_var=0.02)
    out = reference(case, horizon=3, **noise)
    T, F, S, C = case["T"], case["F"], case["S"], out["sm_id"].shape[0]
    worst, checked, filled = 0.0, 0, 0
    for s in range(S):
        for i in range(int(case["num_tracks"][s])):
            fi, la = int(case["track_first"][s, i]), int(case["track_last"][s, i])
            z, seen = np.zeros((la - fi + 1, 4)), np.zeros(la - fi + 1, bool)
            for f in range(fi, la + 1):
                j = np.nonzero(case["track_id"][:int(np.clip(case["n"][s * F + f], 0, T)), s * F + f] == i)[0]
                if len(j):
                    z[f - fi], seen[f - fi] = case["where"][j[0], s * F + f].astype(np.float64), True
            assert seen[0] and seen[-1]
            cols = [matrix_smoother(z[:, c], seen, noise["process_noise"][0 if c % 2 else 1], 5e-4, 0.02) for c in range(4)]
            exact = _exact_where(case, out, noise, s, i)
            for f in range(fi, la + 1):
                row = np.nonzero(out["sm_id"][:, s * F + f] == i)[0]
                assert len(row) == 1
                want = np.array([cols[c][0][f - fi] for c in range(4)])
                worst = max(worst, np.abs(exact[f] - want).max())
                vel = np.array([IMG[1] * cols[1][1][f - fi] * 0.5, IMG[0] * cols[3][1][f - fi] * 0.5])
                assert np.allclose(out["sm_velocity"][row[0], s * F + f], vel, rtol=1e-5, atol=1e-6)
                assert out["sm_state"][row[0], s * F + f] == (OBSERVED if seen[f - fi] else FILLED)
                checked += 1
                filled += 0 if seen[f - fi] else 1
            if F - 1 - la <= max_age:                              # the forecast: filtered state at `last`, shifts only
                row = np.nonzero(out["fc_id"][:, s * 3] == i)[0]
                assert len(row) == 1
                for k in (1, 2, 3):
                    m = F - 1 - la + k
                    want = np.array([cols[0][2][0], cols[1][2][0] + m * cols[1][2][1], cols[2][2][0], cols[3][2][0] + m * cols[3][2][1]])
                    got = out["fc_where"][row[0], s * 3 + k - 1].astype(np.float64)
                    assert np.abs(got - want).max() <= 1e-12 + 6e-8 * np.abs(want).max()      # (+ one fp32 rounding of the output)
    print("tracks' frames checked %d, filled %d, worst float64 difference %.3g" % (checked, filled, worst))
    assert worst <= 1e-12 and checked > 20 and (filled > 0) == (max_age > 0)


def _exact_where(case, out, noise, s, i):
    """the float64 smoothed values of one track, straight from the module's own recursion (sm_where is that rounded to fp32)"""
    F, T = case["F"], case["T"]
    fi, la = int(case["track_first"][s, i]), int(case["track_last"][s, i])

    def z_of(f):
        j = np.nonzero(case["track_id"][:int(np.clip(case["n"][s * F + f], 0, T)), s * F + f] == i)[0]
        return case["where"][j[0], s * F + f].astype(np.float64) if len(j) else None

    q = np.array([noise["process_noise"][1], noise["process_noise"][0]] * 2)
    xs, vs, _ = trajectory._smooth_track(z_of, fi, la, q, noise["measurement_noise"], noise["velocity_var"])
    for f in range(fi, la + 1):                                    # and sm_where is exactly its fp32 rounding
        row = np.nonzero(out["sm_id"][:, s * F + f] == i)[0][0]
        assert np.array_equal(bits(out["sm_where"][row, s * F + f]), bits(xs[f].astype(np.float32)))
    return xs


def test_exact_invariants_one_sighting_and_constant_tracks():
    case = jumping_case()
    out = reference(case, horizon=2)
    T, F = case["T"], case["F"]
    assert (out["sm_count"] == T).all() and (out["sm_state"][:T] == OBSERVED).all() and (out["sm_state"][T:] == ABSENT).all()
    for f in range(F):                                             # one sighting: the `where` bits, whatever the noise settings
        for row in range(T):
            j = int(out["sm_src_slot"][row, f])
            assert out["sm_src_frame"][row, f] == f and case["track_id"][j, f] == out["sm_id"][row, f]
            assert np.array_equal(bits(out["sm_where"][row, f]), bits(case["where"][j, f]))
            assert np.array_equal(bits(out["sm_boxes"][row, f]), bits(case["boxes"][j, f]))
    assert (out["sm_velocity"] == 0).all()
    # a track whose sightings all carry one value (with a gap): that value bit for bit, v = 0, in the filled frame and the forecast too
    w = (np.float32(0.3), np.float32(0.123456789), np.float32(0.31), np.float32(-0.2222222))
    frames = [[(w, 0.9, 1.0)], [(w, 0.9, 1.0)], [], [(w, 0.9, 1.0)], [(w, 0.9, 1.0)]]
    const = with_tracker(rows_from_objects(frames, 2, 3, 4), 5, 1)
    assert const["num_tracks"].tolist() == [1]
    for noise in (dict(), dict(process_noise=(0.7, 3e-9), measurement_noise=1e-7, velocity_var=11.0)):
        o = reference(const, horizon=4, **noise)
        assert o["sm_state"][0].tolist() == [OBSERVED, OBSERVED, FILLED, OBSERVED, OBSERVED] and (o["sm_state"][1:] == ABSENT).all()
        assert all(np.array_equal(bits(o["sm_where"][0, f]), bits(np.array(w))) for f in range(5))
        assert all(np.array_equal(bits(o["fc_where"][0, k]), bits(np.array(w))) for k in range(4))
        assert (o["sm_velocity"] == 0).all() and (o["fc_velocity"] == 0).all() and (o["fc_state"][0] == FORECAST).all()
        assert (o["sm_src_frame"][0].tolist(), o["sm_src_slot"][0].tolist()) == ([0, 1, 1, 3, 4], [0] * 5)
        assert o["sm_counts"].tolist() == [[2 * 5 * 2 - 5, 4, 1]]


@pytest.mark.parametrize("T,F,S,max_age,seed", [(3, 8, 3, 1, 4), (3, 5, 1, 2, 5), (6, 17, 2, 2, 6), (32, 6, 1, 1, 7), (3, 8, 2, 0, 8),
                                                (12, 9, 2, 3, 9)])
def test_rows_bound_order_sources_and_counts_on_random_churn(T, F, S, max_age, seed):
    case = drifting_case(T, F, S, max_age, seed=seed, dropout=0.35)
    out = reference(case, horizon=2)
    C = trajectory.completed_rows(T, max_age)
    assert out["sm_id"].shape == (C, S * F)
    spanning_total = 0
    for s in range(S):
        n_tr = int(case["num_tracks"][s])
        first, last = case["track_first"][s, :n_tr], case["track_last"][s, :n_tr]
        for f in range(F):
            r = s * F + f
            want = [i for i in range(n_tr) if first[i] <= f <= last[i]]
            assert len(want) <= C                                  # the row bound n_f <= C
            spanning_total += len(want)
            assert out["sm_count"][r] == len(want) and out["sm_id"][:len(want), r].tolist() == want      # ascending id
            assert (out["sm_id"][len(want):, r] == -1).all() and (out["sm_state"][len(want):, r] == ABSENT).all()
            assert (out["sm_where"][len(want):, r] == 0).all() and (out["sm_boxes"][len(want):, r] == 0).all()
            n = int(np.clip(case["n"][r], 0, T))
            for row, i in enumerate(want):
                here = [j for j in range(n) if case["track_id"][j, r] == i]
                if here:
                    assert out["sm_state"][row, r] == OBSERVED and (out["sm_src_frame"][row, r], out["sm_src_slot"][row, r]) == (f, here[0])
                else:                                              # FILLED: the latest sighting before f
                    assert out["sm_state"][row, r] == FILLED and max_age > 0
                    g = int(out["sm_src_frame"][row, r])
                    assert f - max_age <= g < f and case["track_id"][out["sm_src_slot"][row, r], s * F + g] == i
                    assert all(i not in case["track_id"][:, s * F + h] for h in range(g + 1, f))
                assert np.array_equal(bits(out["sm_boxes"][row, r]), bits(scene_boxes(out["sm_where"][row, r], IMG)))
                src = (out["sm_src_slot"][row, r], s * F + out["sm_src_frame"][row, r])
                assert np.array_equal(bits(out["sm_what"][row, r]), bits(case["what"][src]))
                assert np.array_equal(bits(out["sm_glimpse"][row, r]), bits(case["glimpse"][src])) and out["sm_score"][row, r] == case["score"][src]
        live = [i for i in range(n_tr) if F - 1 - last[i] <= max_age]
        for k in range(2):
            assert out["fc_count"][s * 2 + k] == len(live) <= C and out["fc_id"][:len(live), s * 2 + k].tolist() == live
            assert (out["fc_state"][:len(live), s * 2 + k] == FORECAST).all() and (out["fc_state"][len(live):, s * 2 + k] == ABSENT).all()
            assert out["fc_src_frame"][:len(live), s * 2 + k].tolist() == [int(last[i]) for i in live]
    assert out["sm_counts"].sum() == C * F * S and out["sm_counts"][:, 1:].sum() == spanning_total
    assert (out["sm_counts"][:, FILLED].sum() == 0) == (max_age == 0 or case["track_gaps"].sum() == 0)
    assert out["sm_counts"][:, FILLED].sum() >= case["track_gaps"].sum()
    print("rows C=%d, spanning %d, filled %d, tracks %s" % (C, spanning_total, out["sm_counts"][:, FILLED].sum(), case["num_tracks"].tolist()))


def test_full_table_and_a_track_born_in_the_last_frame():
    full = full_table_case()
    out = reference(full, horizon=1)
    assert out["sm_id"].shape[0] == 32 and (out["sm_count"] == 32).all() and (out["fc_count"] == 32).all()
    assert out["sm_id"][:, 1].tolist() == list(range(32)) and out["sm_counts"].tolist() == [[0, 64, 0]]
    case = drifting_case(3, 5, 1, 1, seed=12)
    born = [i for i in range(int(case["num_tracks"][0])) if case["track_first"][0, i] == 4]
    assert born                                                    # a track of one frame, the last: forecast from v = 0
    out = reference(case, horizon=3)
    i = born[-1]
    row = out["fc_id"][:, 0].tolist().index(i)
    rr = out["sm_id"][:, 4].tolist().index(i)
    assert all(np.array_equal(bits(out["fc_where"][row, k]), bits(out["sm_where"][rr, 4])) for k in range(3))


def test_planted_line_is_filled_and_forecast_within_the_stated_error():
    """the defaults on a planted line of step 1 / 16 on tx with one frame missing: the filled row within 2e-4 of the line (0.005 px of
    box position at W = 50), the three-frame forecast within 1e-4"""
    case, gt, gt_future, gaps = planted_sequences()
    out = reference(case, horizon=PLANTED["HZ"])
    S, F, K = PLANTED["S"], PLANTED["F"], PLANTED["K"]
    fill_err, fc_err, n_filled = 0.0, 0.0, 0
    for s in range(S):
        for f in range(F):
            for row in range(int(out["sm_count"][s * F + f])):
                if out["sm_state"][row, s * F + f] == FILLED:
                    o = int(out["sm_id"][row, s * F + f])          # (ids are issued in slot order: id == object here)
                    fill_err = max(fill_err, np.abs(out["sm_where"][row, s * F + f].astype(np.float64) - np.array(planted_where(s, o, f))).max())
                    n_filled += 1
        for k in range(PLANTED["HZ"]):
            for row in range(K):
                o = int(out["fc_id"][row, s * PLANTED["HZ"] + k])
                fc_err = max(fc_err, np.abs(out["fc_where"][row, s * PLANTED["HZ"] + k].astype(np.float64) - np.array(planted_where(s, o, F + k))).max())
    print("filled rows %d, worst |where - line| %.3g; forecast worst %.3g" % (n_filled, fill_err, fc_err))
    assert n_filled == gaps and fill_err <= 2e-4 and fc_err <= 1e-4


def test_identity_figures_of_the_planted_sequences():
    case, gt, gt_future, gaps = planted_sequences()
    out = reference(case, horizon=PLANTED["HZ"])
    F, tau = PLANTED["F"], PLANTED["TAU"]
    raw = track.reference_score(case["boxes"], case["n"], case["track_id"], gt, F, tau)
    done = track.reference_score(out["sm_boxes"], out["sm_count"], out["sm_id"], gt, F, tau)
    c = lambda res, k: int(res["seq_counts"][:, track.COUNTS.index(k)].sum())
    assert c(raw, "misses") == gaps and c(done, "misses") == 0                # exactly one miss per planted gap; none after completion
    assert c(raw, "fp") == c(done, "fp") == 0 and c(raw, "idsw") == c(done, "idsw") == 0
    assert c(raw, "gt") == c(done, "gt") == PLANTED["S"] * F * PLANTED["K"]
    mota = lambda res: track.mot_summary(res["seq_counts"].sum(0), res["seq_iou"].sum())["mota"]
    assert mota(done) == 1.0 > mota(raw) == 1.0 - gaps / c(raw, "gt")
    ahead = track.reference_score(out["fc_boxes"], out["fc_count"], out["fc_id"], gt_future, PLANTED["HZ"], tau)
    assert c(ahead, "misses") == 0 and c(ahead, "fp") == 0 and c(ahead, "matches") == PLANTED["S"] * PLANTED["HZ"] * PLANTED["K"]


def test_non_finite_sightings_stay_in_their_track():
    """a NaN `where` value poisons the components it touches of that track, and nothing else"""
    case, _, _, _ = planted_sequences()
    r = 3
    j = int(np.nonzero(case["track_id"][:, r] == 0)[0][0])
    case["where"][j, r, 1] = np.nan                                # tx of track 0 in sequence 0
    out = reference(case, horizon=2)
    F = PLANTED["F"]
    assert np.isnan(out["sm_where"][0, :F, 1]).all() and np.isfinite(out["sm_where"][0, :F, [0, 2, 3]]).all()
    assert np.isfinite(out["sm_where"][1, :F]).all() and np.isfinite(out["sm_where"][:, F:]).all()
    assert np.isnan(out["fc_where"][0, :2, 1]).all() and np.isfinite(out["fc_where"][1]).all()


def test_binding_header_and_build_list():
    from attend_infer_repeat_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "air_hip.h")).read()
    for name, n_args in (("air_track_smooth", 39), ("air_track_fill", 18)):
        m = re.search(r"AIR_ENGINE_API int %s\(([^;]*)\);" % name, text)
        assert m, "%s is not declared AIR_ENGINE_API" % name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
    assert _lib.SIGNATURES["air_track_smooth_workspace_bytes"][0] is _lib.c_size_t
    assert "trajectory_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "trajectory_kernels.hip"))
    assert re.search(r"#define AIR_ABI_VERSION 10\b", text) and re.search(r"#define AIR_ENGINE_ABI_VERSION 5\b", text)
    src = open(os.path.join(build.CSRC, "trajectory_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd(&a.sm_where" not in src
    lib = _lib.load()                                              # the size entry is host code: callable without a GPU
    assert lib.air_track_smooth_workspace_bytes(6, 1024) == 28 * 8 * 6 * 1024 and lib.air_track_smooth_workspace_bytes(33, 4) == 0
