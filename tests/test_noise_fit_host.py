"""Group Nf on the CPU: the likelihood statistics behind trajectory.TrajectoryNoiseFitter (tests/noise_fit_cases.py holds the exact
routes, the restatement with its defects, the sweep and the cases).
  1  the two exact routes agree exactly (the prediction-error decomposition);
  2  trajectory.reference_noise_stats against the exact values: the recorded sweep and the bound derived from it;
  3  every planted defect moves a statistic by DEFECT_MARGIN x the bound;
  4  the concentration identity: profile_loglik at r^ is the surface, and the direct sum of the smoother's own filter at the fitted terms;
  5  recovery of planted noise terms from simulated tracks, with the reference alone;
  6  the refusals of check_fit_arguments and of the library entries mirror each other, before any launch;
  7  the arg-max rules and the ValueErrors of profile_fit."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import noise_fit_cases as NC
import smoother_cases as SC

from attend_infer_repeat_amd import trajectory

NU = trajectory.default_velocity_ratio()


# ---- 1. exact, two routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", (1e-29, 0.0625, 4.0, 1e15))
def test_the_two_exact_routes_agree_exactly(rho):
    """both noise classes run the same statements with their own rho: every rho here serves as either"""
    for label, z, seen in NC.exact_tracks():
        for nu in (0.0, NU):
            one, two = NC.exact_filter_stats(z, seen, rho, nu), NC.exact_dense_stats(z, seen, rho, nu)
            assert one == two, (label, rho, nu)
            assert one[2] == int(seen[1:].sum())
    label, z, seen = NC.exact_tracks()[-1]
    assert label == "constant" and NC.exact_filter_stats(z, seen, rho, NU)[0] == 0
    assert NC.exact_tracks()[0][2].sum() == 2 and max(len(z) for _, z, _ in NC.exact_tracks()) == 24


# ---- 2. the restatement against exact -----------------------------------------------------------------------------------------------------------
def test_the_reference_is_the_exact_statistic_within_the_bound():
    """the part of the sweep the suite repeats; the worst values it shows must not pass the record the bound is derived from"""
    worst_q, worst_l = (0.0, None), (0.0, None)
    for pt in NC.sweep_points("test"):
        label, rho, nu, eq, el = NC.sweep_errors(pt)
        worst_q, worst_l = max(worst_q, (eq, (label, rho, nu))), max(worst_l, (el, (label, rho, nu)))
    print("\n  worst relative error: Q %.3g at %s, log Pi %.3g at %s; bounds %.3g / %.3g"
          % (worst_q + worst_l + (NC.BOUND_Q, NC.BOUND_LOG_PI)))
    assert worst_q[0] <= NC.FULL_SWEEP["q"] * 1.05 and worst_l[0] <= NC.FULL_SWEEP["log_pi"] * 1.05      # (the record is rounded to two digits)
    assert worst_q[0] <= NC.BOUND_Q and worst_l[0] <= NC.BOUND_LOG_PI
    assert 70 < NC.MARGIN < 72                                     # smoother_cases: 0.25 units over its worst 3.5e-3


def test_the_scalar_restatement_is_the_reference_bit_for_bit():
    """noise_fit_cases.restated (what the defects are planted in) and trajectory.reference_noise_stats share no statement"""
    case = NC.gpu_case("small")
    shift, scale, nu = NC.grid_rows()["g5"]
    out = NC.reference_totals(case, shift, scale, nu)
    t = case["seqs"][0][1]                                         # sequence 0, id 1: "1010011" from frame 1 on -- it alone, for candidate 2
    where = np.zeros((1, 8, 4), np.float32)
    where[0, 1:] = t["z"]
    one = trajectory.reference_noise_stats(where, np.r_[0, t["seen"]].astype(np.int32), np.zeros((1, 8), np.int32), [1], [[1] + [-1] * 7],
                                           [[7] + [-1] * 7], 8, shift, scale, nu)
    z = t["z"].astype(np.float64)
    for c, (ca, cb), rho in ((0, (1, 3), shift), (1, (0, 2), scale)):
        for g in range(5):
            Q, m, k, n = NC.restated(z[:, ca], z[:, cb], t["seen"], rho[g], nu)
            assert (Q, m, k, n) == (one["q"][0, g, c], one["m"][0, g, c], one["k"][0, g, c], one["n"][0]), (c, g)
    assert out["n"].tolist() == [7 + 3 + 0 + 1, 3 + 3 + 0, 0]


# ---- 3. planted defects -----------------------------------------------------------------------------------------------------------------------
def _moved(a, b):
    """the larger relative move of (Q, log Pi) between two (Q, m, k, n), each in units of its bound"""
    la, lb = math.log(a[1]) + a[2] * math.log(2.0), math.log(b[1]) + b[2] * math.log(2.0)
    return max(abs(a[0] - b[0]) / abs(b[0]) / NC.BOUND_Q, abs(la - lb) / abs(lb) / NC.BOUND_LOG_PI)


@pytest.mark.parametrize("defect", NC.DEFECTS + NC.PROFILE_DEFECTS)
def test_a_planted_defect_moves_a_statistic_by_a_margin(defect):
    label, z, seen = NC.exact_tracks()[3]                          # span 24 with a gap of 3
    zb = 0.5 * z + 0.1
    rho, rho_other = 0.0625, 1e-3
    clean = NC.restated(z, zb, seen, rho, NU)
    exact = [NC.exact_filter_stats(c, seen, rho, NU) for c in (z, zb)]
    Qe, le = float(exact[0][0] + exact[1][0]), NC.log_fraction(exact[0][1])
    assert abs(clean[0] - Qe) / Qe <= NC.BOUND_Q and abs(math.log(clean[1]) + clean[2] * math.log(2.0) - le) / le <= NC.BOUND_LOG_PI
    if defect in NC.PROFILE_DEFECTS:
        totals = {k: v for k, v in NC.reference_totals(NC.gpu_case("small"), (rho,), (rho_other,), NU).items() if k.startswith("tot_")}
        good, bad = NC.restated_profile(totals, 0, 0), NC.restated_profile(totals, 0, 0, defect)
        assert good == trajectory.profile_fit(totals, (rho,), (rho_other,), NU)["loglik"]
        moved = abs(bad - good) / abs(good) / max(NC.BOUND_Q, NC.BOUND_LOG_PI)
    else:
        moved = _moved(NC.restated(z, zb, seen, rho, NU, defect=defect, rho_other=rho_other), clean)
    print("\n  %s: %.3g bounds" % (defect, moved))
    assert moved >= NC.DEFECT_MARGIN


# ---- 4. the concentration identity --------------------------------------------------------------------------------------------------------------
def _direct_loglik(case, fit):
    """-1/2 sum (log 2 pi s + e^2 / s) over every update of every track and component, from trajectory._filter_step -- the smoother's
    own restated filter -- at the ABSOLUTE fitted terms; and the sum of the terms' magnitudes (what a rounding-only tolerance scales with)"""
    (qs, qc), r, vv = fit["process_noise"], fit["measurement_noise"], fit["velocity_var"]
    q = np.array([qc, qs, qc, qs])
    total, mag = 0.0, 0.0
    for s, tracks in enumerate(case["seqs"]):
        for t in tracks:
            z = t["z"].astype(np.float64)
            filt = trajectory._filter_start(z[0], r, vv)
            for f in range(1, len(z)):
                pred, filt = trajectory._filter_step(filt, z[f] if t["seen"][f] else None, q, r)
                if t["seen"][f]:
                    sn, e = pred[2] + r, z[f] - pred[0]
                    terms = np.log(2.0 * np.pi * sn) + e * e / sn
                    total, mag = total - 0.5 * float(terms.sum()), mag + 0.5 * float(np.abs(np.log(2.0 * np.pi * sn)).sum() + (e * e / sn).sum())
    return total, mag


def test_the_concentration_identity():
    case = NC.gpu_case("small")
    shift, scale, nu = (1e-3, 0.0625, 4.0), (0.25, 1e-2, 1e-5), NU
    totals = NC.reference_totals(case, shift, scale, nu)
    fit = trajectory.profile_fit(totals, shift, scale, nu)
    N = fit["n_innovations"]
    assert N == 4 * int(totals["n"].sum()) == 4 * 17
    for i in range(3):
        for j in range(3):
            Q = totals["tot_q"][i, 0] + totals["tot_q"][j, 1]
            r_hat = Q / N
            at_r, surf = trajectory.profile_loglik(totals, i, j, r_hat), fit["surface"][i, j]
            _, mag = _direct_loglik(case, dict(process_noise=(r_hat * shift[i], r_hat * scale[j]), measurement_noise=r_hat, velocity_var=r_hat * nu))
            # rounding only: three terms of magnitude <= mag + N each carry a few ulp; the two formulas differ by nothing else
            assert abs(at_r - surf) <= 16 * np.finfo(float).eps * (mag + N), (i, j, at_r, surf)
            assert trajectory.profile_loglik(totals, i, j, 1.7 * r_hat) < surf and trajectory.profile_loglik(totals, i, j, r_hat / 1.7) < surf
    i, j = fit["cell"]
    direct, mag = _direct_loglik(case, fit)
    # the direct sum's Q / r and Lambda are each within the sweep's relative bound of exact, as the reference's are: twice the bound
    tol = 2.0 * max(NC.BOUND_Q, NC.BOUND_LOG_PI) * mag
    print("\n  surface %.12g, direct sum %.12g, difference %.3g, tolerance %.3g" % (fit["loglik"], direct, abs(direct - fit["loglik"]), tol))
    assert abs(direct - fit["loglik"]) <= tol


# ---- 5. recovery ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", NC.RECOVERY_SEEDS)
def test_planted_noise_terms_are_recovered(seed):
    """a condition on the estimator, checked with the reference alone: 192 tracks of 16 frames drawn from the model with the truth on
    a node of the default grid, 10 % of the inner frames unseen, fp32 sightings"""
    case, grid, nu = NC.simulated_case(seed), trajectory.DEFAULT_FIT_RATIOS, NC.TRUTH["velocity_ratio"]
    assert len(grid) == 19 and grid[0] == 1e-6 and grid[-1] == 1e3 and grid[10] == NC.TRUTH["shift_ratio"] and grid[8] == NC.TRUTH["scale_ratio"]
    evaluate = lambda a, b: {k: v for k, v in NC.reference_totals(case, a, b, nu).items() if k in trajectory.TOTAL_KEYS}
    fit = trajectory.fit_with_zoom(evaluate, grid, grid, nu)
    print("\n  seed %d: cell %s, r^ / r = %.4f, loglik / N = %.4f" % (seed, fit["cell"], fit["measurement_noise"] / NC.TRUTH["r"],
                                                                     fit["loglik"] / fit["n_innovations"]))
    assert abs(fit["cell"][0] - 10) <= 1 and abs(fit["cell"][1] - 8) <= 1 and fit["on_edge"] == (False, False)
    assert 1.0 / NC.R_FACTOR <= fit["measurement_noise"] / NC.TRUTH["r"] <= NC.R_FACTOR
    assert 1.0 / NC.R_FACTOR_SEEN <= fit["measurement_noise"] / NC.TRUTH["r"] <= NC.R_FACTOR_SEEN       # the record itself
    trajectory.check_arguments(3, 16, None, **{k: fit[k] for k in trajectory.FIT_KEYS})
    if seed == NC.RECOVERY_SEEDS[0]:
        zoomed = trajectory.fit_with_zoom(evaluate, grid, grid, nu, zoom=2, totals=fit["totals"])
        assert zoomed["loglik"] >= fit["loglik"]
        assert grid[9] <= zoomed["process_noise"][0] / zoomed["measurement_noise"] <= grid[11]
        # the value at the current defaults, comparable on the same tracks
        D = trajectory.DEFAULTS
        at = evaluate((D["process_noise"][0] / D["measurement_noise"],), (D["process_noise"][1] / D["measurement_noise"],))
        assert trajectory.profile_loglik(at, 0, 0, D["measurement_noise"]) < fit["loglik"]


def test_accumulation_over_calls_is_one_call_over_all():
    """two calls with the totals passed on = the sequences of both combined in ascending order; accumulate=False restarts"""
    a, b = NC.gpu_case("small"), NC.gpu_case("foreign")
    shift, scale, nu = NC.grid_rows()["g5"]
    one = NC.reference_totals(a, shift, scale, nu)
    two = NC.reference_totals(b, shift, scale, nu, totals=one)
    both = trajectory.reference_noise_reduce(np.concatenate([one["q"], two["q"]]), np.concatenate([one["m"], two["m"]]),
                                             np.concatenate([one["k"], two["k"]]), np.concatenate([one["n"], two["n"]]))
    assert two["tot_n"][0] == both["tot_n"][0] == one["n"].sum() + two["n"].sum()
    assert np.array_equal(two["tot_k"], both["tot_k"]) and np.allclose(two["tot_q"], both["tot_q"], rtol=1e-14, atol=0)
    again = NC.reference_totals(b, shift, scale, nu, totals=one, accumulate=False)
    alone = NC.reference_totals(b, shift, scale, nu)
    for k in trajectory.TOTAL_KEYS:
        assert np.array_equal(again[k], alone[k]), k
    fresh = trajectory.reference_noise_reduce(one["q"], one["m"], one["k"], one["n"], trajectory.new_noise_totals(5))
    for k in trajectory.TOTAL_KEYS:                                # the identities: combining into empty totals is writing
        assert np.array_equal(fresh[k], one[k]), k


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def _stats_status(lib, x, T=3, S=2, F=4, R=8, shift=(0.25,), scale=(0.25,), nu=100.0, where=None, G=None, null=None):
    """air_track_noise_stats with every pointer valid host memory and `where` 4 bytes off alignment: a call the checks in front let
    through is refused with AIR_E_ALIGN (-3), before any launch"""
    arr = ctypes.c_double * max(len(shift), 1)
    a, b = arr(*shift), arr(*scale)
    ptrs = [ctypes.c_void_p(x.value + 4) if where is None else where] + [x] * 5
    outs = [x] * 4
    if null is not None:
        (ptrs if null < 6 else outs)[null % 6] = None
    return lib.air_track_noise_stats(*ptrs, T, S, F, R, len(shift) if G is None else G, a, b, float(nu), *outs, None)


def test_the_refusals_in_python_and_in_the_library_mirror_each_other():
    from attend_infer_repeat_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    x = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)
    lo, hi, vhi = trajectory.FIT_Q_OVER_R_MIN, trajectory.FIT_Q_OVER_R_MAX, trajectory.FIT_V_OVER_R_MAX
    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, 0.0)))
    inside = [dict(), dict(shift=(lo, hi), scale=(hi, lo)), dict(nu=0.0), dict(nu=vhi), dict(shift=(1.0,) * 32, scale=(2.0,) * 32)]
    for kw in inside:                                              # the limits themselves included
        trajectory.check_fit_arguments(3, 4, 8, kw.get("shift", (0.25,)), kw.get("scale", (0.25,)), kw.get("nu", 100.0))
        assert _stats_status(lib, x, **kw) == -3, kw
    outside = [(dict(shift=(up(hi),)), "FIT_Q_OVER_R_MAX"), (dict(scale=(1.0, up(hi)), shift=(1.0, 1.0)), "FIT_Q_OVER_R_MAX"),
               (dict(shift=(down(lo),)), "FIT_Q_OVER_R_MIN"), (dict(scale=(down(lo),)), "FIT_Q_OVER_R_MIN"),
               (dict(nu=up(vhi)), "FIT_V_OVER_R_MAX"), (dict(nu=-1.0), "velocity_ratio"), (dict(nu=float("nan")), "velocity_ratio"),
               (dict(shift=(float("nan"),)), "shift_ratios"), (dict(scale=(0.0,)), "scale_ratios"),
               (dict(shift=(1.0,) * 33, scale=(1.0,) * 33), "1..32 candidates")]
    for kw, words in outside:
        with pytest.raises(ValueError, match=words):
            trajectory.check_fit_arguments(3, 4, 8, kw.get("shift", (0.25,)), kw.get("scale", (0.25,)), kw.get("nu", 100.0))
        assert _stats_status(lib, x, **kw) == -2, kw
    with pytest.raises(ValueError, match="same number"):
        trajectory.check_fit_arguments(3, 4, 8, (1.0, 2.0), (1.0,))
    assert _stats_status(lib, x, G=0) == -2
    # the shapes air_track_smooth refuses, by the words of track.check_arguments
    for kw, words in ((dict(T=33), "max_steps"), (dict(T=0), "max_steps"), (dict(F=0, R=0), "n_frames"), (dict(R=9), "no multiple"),
                      (dict(T=32, F=1024, R=2048), "int16")):
        a = dict(dict(T=3, S=2, F=4, R=8), **kw)
        with pytest.raises(ValueError, match=words):
            trajectory.check_fit_arguments(a["T"], a["F"], a["R"])
        assert _stats_status(lib, x, **a) == -2, kw
    assert _stats_status(lib, x, S=0, R=0) == -2 and _stats_status(lib, x, T=32, S=2 ** 27, F=1, R=2 ** 27) == -2
    for null in range(10):
        assert _stats_status(lib, x, null=null) == -1, null
    assert lib.air_track_noise_stats(*[x] * 6, 3, 2, 4, 8, 1, None, x, 100.0, *[x] * 4, None) == -1
    off2 = ctypes.c_void_p(x.value + 2)
    red = lambda *a: lib.air_track_noise_reduce(*a, None)
    assert red(x, x, x, x, 2, 5, 1, x, x, x, off2) == -3 and red(x, x, off2, x, 2, 5, 1, x, x, x, x) == -3
    assert red(x, x, x, x, 0, 5, 1, x, x, x, off2) == -2 and red(x, x, x, x, 2, 0, 1, x, x, x, off2) == -2
    assert red(x, x, x, x, 2, 33, 0, x, x, x, off2) == -2 and red(x, x, x, x, 2, 5, 2, x, x, x, off2) == -2
    for null in range(8):
        a = [x] * 4 + [2, 5, 1] + [x] * 4
        a[null if null < 4 else null + 3] = None
        assert red(*a) == -1, null
    assert all(v == 0.0 for v in buf)                              # nothing was written
    # every limit is read from one place: the smoother's
    assert (lo, hi, vhi) == (trajectory.Q_OVER_R_MIN, trajectory.Q_OVER_R_MAX, trajectory.V_OVER_R_MAX)
    src = open(os.path.join(os.path.dirname(trajectory.__file__), "csrc", "noise_fit_kernels.hip")).read()
    for macro, value in (("NFIT_Q_OVER_R_MIN", lo), ("NFIT_Q_OVER_R_MAX", hi), ("NFIT_V_OVER_R_MAX", vhi),
                         ("NFIT_MAX_G", trajectory.FIT_MAX_CANDIDATES)):
        m = re.search(r"#define %s (\S+)" % macro, src)
        assert m and float(m.group(1)) == value, macro


# ---- 7. the arg-max, the errors -------------------------------------------------------------------------------------------------------------------
def _totals(q0, q1, n=5, m=0.75, k=3):
    G = len(q0)
    return {"tot_q": np.array([q0, q1], np.float64).T.copy(), "tot_m": np.full((G, 2), m), "tot_k": np.full((G, 2), k, np.int64),
            "tot_n": np.array([n], np.int64)}


def test_the_arg_max_takes_the_lowest_cell_of_a_tie_and_never_a_nan():
    g = (0.1, 1.0, 10.0)
    fit = trajectory.profile_fit(_totals([2.0, 1.0, 1.0], [3.0, 1.0, 1.0]), g, g, NU)
    assert fit["cell"] == (1, 1) and fit["on_edge"] == (False, False)     # (1, 1), (1, 2), (2, 1), (2, 2) tie: the lowest row-major
    nan = float("nan")
    fit = trajectory.profile_fit(_totals([nan, 2.0, 1.0], [1.0, nan, 1.0]), g, g, NU)
    assert fit["cell"] == (2, 0) and fit["on_edge"] == (True, True) and np.isnan(fit["surface"][0]).all() and np.isnan(fit["surface"][:, 1]).all()
    assert fit["measurement_noise"] == 2.0 / 20 and fit["n_innovations"] == 20 and fit["process_noise"] == (0.1 * 10.0, 0.1 * 0.1)
    assert fit["velocity_var"] == 0.1 * NU and fit["loglik"] == fit["surface"][2, 0]
    assert set(fit) == {"process_noise", "measurement_noise", "velocity_var", "loglik", "n_innovations", "cell", "on_edge", "surface"}
    trajectory.check_arguments(3, 4, 8, **{k: fit[k] for k in trajectory.FIT_KEYS})
    with pytest.raises(ValueError, match="NaN in every cell"):
        trajectory.profile_fit(_totals([nan] * 3, [1.0] * 3), g, g, NU)


def test_the_errors_of_profile_fit_are_in_words():
    g = (0.1, 1.0)
    with pytest.raises(ValueError, match="no track with two sightings"):
        trajectory.profile_fit(_totals([0.0, 0.0], [0.0, 0.0], n=0), g, g, NU)
    with pytest.raises(ValueError, match="every innovation is zero"):
        trajectory.profile_fit(_totals([0.0, 0.0], [0.0, 0.0]), g, g, NU)
    with pytest.raises(ValueError, match="supported domain.*R_MIN"):       # r^ = 1e-150 / 20
        trajectory.profile_fit(_totals([1e-150, 1e-150], [1e-150, 1e-150]), g, g, NU)
    with pytest.raises(ValueError, match="supported domain.*R_MAX"):       # r^ = 1e140 / 20
        trajectory.profile_fit(_totals([1e140, 1e140], [1e140, 1e140]), g, g, NU)
    with pytest.raises(ValueError, match="hold 2 candidates"):
        trajectory.profile_fit(_totals([1.0, 1.0], [1.0, 1.0]), (1.0,), (1.0,), NU)
    with pytest.raises(ValueError, match="zoom"):
        trajectory.fit_with_zoom(lambda a, b: None, g, g, NU, zoom=-1)
    # a constant track alone: the device's statistic is exactly zero, and the fit says so
    z = np.full((4, 4), 0.5, np.float32)
    case = SC.planted_case(4, 1, 0, [[dict(first=0, seen=np.ones(4, bool), z=z)]])
    totals = NC.reference_totals(case, g, g, NU)
    assert (totals["tot_q"] == 0.0).all() and totals["tot_n"][0] == 3
    with pytest.raises(ValueError, match="every innovation is zero"):
        trajectory.profile_fit(totals, g, g, NU)


def test_the_zoom_grid_keeps_the_incumbent_and_the_domain():
    g = trajectory.DEFAULT_FIT_RATIOS
    z = trajectory.zoom_grid(g, 10)
    assert len(z) == 19 and z[0] == g[9] and z[-1] == g[11] and g[10] in z and list(z) == sorted(z)
    lo = trajectory.zoom_grid(g, 0)
    assert lo[0] == g[0] and lo[-1] == g[1]
    assert trajectory.zoom_grid((0.5,), 0) == (0.5,)
    ends = (trajectory.FIT_Q_OVER_R_MIN, 1.0, trajectory.FIT_Q_OVER_R_MAX)
    for best in range(3):
        trajectory.check_fit_arguments(3, 4, 8, trajectory.zoom_grid(ends, best), ends)


def test_the_fit_key_is_a_key_of_its_own_and_checks_first():
    from types import SimpleNamespace
    from attend_infer_repeat_amd import stacks
    eng = SimpleNamespace(cfg=SimpleNamespace(max_steps=3), device="cuda:0")
    k = stacks.fit_key(eng, 2, 8)
    assert k == stacks.fit_key(eng, 2, 8, trajectory.DEFAULT_FIT_RATIOS, trajectory.DEFAULT_FIT_RATIOS, NU, smooth=None)
    assert k.fit == (trajectory.DEFAULT_FIT_RATIOS, trajectory.DEFAULT_FIT_RATIOS, NU) and k != stacks.track_key(eng, 2, 8)
    assert k != stacks.fit_key(eng, 2, 8, velocity_ratio=0.0) and k != stacks.fit_key(eng, 2, 8, max_age=2)
    assert (k.S, k.F, k.matching) == (2, 8, "greedy") and dict(k.assoc)["max_age"] == 1
    with pytest.raises(ValueError, match="smooth"):
        stacks.fit_key(eng, 2, 8, smooth=True)
    with pytest.raises(ValueError, match="FIT_V_OVER_R_MAX"):
        stacks.fit_key(eng, 2, 8, velocity_ratio=1e7)
    with pytest.raises(ValueError, match="int16"):
        stacks.fit_key(eng, 2, 20000)
