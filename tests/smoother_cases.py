"""Group Tj: the exact posterior of the trajectory model, the float64 restatement of the kernel's statements with plantable defects,
the sweep that measures the supported noise domain, and the case tables of test_smoother_cases_host.py and test_smoother_kernels.py.

The model (one `where` component): state (x, v), dt = 1, x_f = x_{f-1} + v_{f-1} + w_f / 2, v_f = v_{f-1} + w_f, w_f ~ N(0, q): the Q the
predict step states (q/4, q/2, q).  Prior x_0 ~ N(z_0, r), v_0 ~ N(0, vv) (vv = 0: v_0 = 0 exactly).  Sightings z_f = x_f + N(0, r).  The
posterior mean is the minimiser of one weighted least-squares problem; `exact_posterior` solves its normal equations in
fractions.Fraction and rounds once at the end.  Nothing here shares a statement with trajectory.reference_smooth.

THE UNIT of every error below: 2^-24 max|z| over the track's sightings, about one float32 rounding of an output, for positions, and for
velocities as positions per frame.  THE BOUND is derived, not measured: a float32 output is within one float32 ulp of the rounded exact
value once the float64 value it is rounded from is within half an ulp of the exact one; the float64 restatement is held to 0.25 units
(margin 2)."""
import functools
import math
import os
import sys
from fractions import Fraction

if __name__ == "__main__":                                         # (python tests/smoother_cases.py from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from attend_infer_repeat_amd import trajectory

UNIT = 2.0 ** -24
BOUND = 0.25                                                       # units: what the float64 restatement must stay under inside the box
DEFECT_MARGIN = 4.0                                                # every planted defect: error / BOUND >= this


# ---- 1. the exact posterior -----------------------------------------------------------------------------------------------------------------
def _solve(M, y):
    """Gaussian elimination, exact.  M is symmetric positive definite, so no pivoting is needed: every pivot is a ratio of leading
    minors, all positive.  The Fractions are scaled to integers by their common denominator and eliminated fraction-free (Bareiss:
    every division below is exact), which spares the gcd of every Fraction operation.  Returns (N, det): the solution is N / det."""
    n = len(y)
    den = 1
    for row in M:
        for v in row:
            if v.denominator > den:                                # (the denominators are powers of two: the largest is the lcm)
                den = v.denominator
    for v in y:
        den = max(den, v.denominator)
    A = [[int(v * den) for v in row] + [int(y[i] * den)] for i, row in enumerate(M)]
    assert all(Fraction(A[i][j], den) == M[i][j] for i in range(n) for j in range(n))
    g = 0
    for row in A:
        g = math.gcd(g, *row)
    A = [[v // g for v in row] for row in A]                       # (matrix and right-hand side alike: the solution is the same)
    prev = 1
    for k in range(n):                                             # (the trailing block stays symmetric: the upper triangle is kept)
        top = A[k]
        piv = top[k]
        assert piv > 0
        for i in range(k + 1, n):
            row = A[i]
            f = top[i]
            for j in range(i, n + 1):
                row[j] = (row[j] * piv - f * top[j]) // prev
        prev = piv
    det = A[n - 1][n - 1]                                          # Bareiss leaves the determinant here; u = N / det, N integers
    N = [0] * n
    for k in range(n - 1, -1, -1):
        num = A[k][n] * det - sum(A[k][j] * N[j] for j in range(k + 1, n))
        N[k], rem = divmod(num, A[k][k])
        assert rem == 0
    return N, det


def exact_posterior_fractions(z, seen, q, r, vv):
    """the posterior means (x_f, v_f), f = 0 .. n - 1, as Fractions.  z [n] (read where seen), seen [n] bool with seen[0]; q, r > 0,
    vv >= 0.  Unknowns u = (x_0, [v_0,] w_1 .. w_{n-1}); x_f = x_0 + f v_0 + sum_{j<=f} (f - j + 1/2) w_j, v_f = v_0 + sum_{j<=f} w_j.
    Minimised: (x_0 - z_0)^2 / r + v_0^2 / vv + sum w_j^2 / q + sum_{seen f >= 1} (x_f - z_f)^2 / r, scaled by r."""
    n = len(z)
    assert seen[0] and n >= 1
    qF, rF, vF = Fraction(float(q)), Fraction(float(r)), Fraction(float(vv))
    zF = [Fraction(float(z[f])) if seen[f] else None for f in range(n)]
    has_v = vF > 0
    nv = 1 + (1 if has_v else 0)
    m = nv + n - 1
    half = Fraction(1, 2)

    def x_row(f):                                                  # x_f as a row over u
        a = [Fraction(0)] * m
        a[0] = Fraction(1)
        if has_v:
            a[1] = Fraction(f)
        for j in range(1, f + 1):
            a[nv + j - 1] = Fraction(f - j) + half
        return a

    def v_row(f):
        a = [Fraction(0)] * m
        if has_v:
            a[1] = Fraction(1)
        for j in range(1, f + 1):
            a[nv + j - 1] = Fraction(1)
        return a

    M = [[Fraction(0)] * m for _ in range(m)]
    y = [Fraction(0)] * m
    # the objective times r q vv (r q when v_0 is dropped): every weight is a product of the inputs, a dyadic rational
    w_obs, w_v0, w_w = (qF * vF, rF * qF, rF * vF) if has_v else (qF, None, rF)
    if has_v:
        M[1][1] += w_v0
    for j in range(1, n):
        M[nv + j - 1][nv + j - 1] += w_w
    G = [[0] * m for _ in range(m)]                                # sum over the sightings of (2 x_row)(2 x_row)^T, in integers
    h = [Fraction(0)] * m
    for f in range(n):                                             # (f = 0: the prior on x_0 is a sighting of weight 1 / r)
        if not seen[f]:
            continue
        a = [int(2 * v) for v in x_row(f)]
        nz = [i for i in range(m) if a[i]]
        for i in nz:
            h[i] += a[i] * zF[f]
            Gi, ai = G[i], a[i]
            for k in nz:
                Gi[k] += ai * a[k]
    for i in range(m):
        y[i] = w_obs * h[i] / 2
        for k in range(m):
            if G[i][k]:
                M[i][k] += w_obs * G[i][k] / 4
    N, det = _solve(M, y)                                          # u = N / det
    xs = [Fraction(sum(int(2 * a) * b for a, b in zip(x_row(f), N)), 2 * det) for f in range(n)]
    vs = [Fraction(sum(int(a) * b for a, b in zip(v_row(f), N)), det) for f in range(n)]
    return xs, vs


def exact_posterior(z, seen, q, r, vv):
    """(xs, vs) float64 [n]: the exact posterior means rounded once"""
    xs, vs = exact_posterior_fractions(z, seen, q, r, vv)
    return np.array([float(v) for v in xs]), np.array([float(v) for v in vs])


def exact_filtered(z, seen, q, r, vv, upto):
    """the exact FILTERED mean (x, v) at frame `upto`: the same solve restricted to the frames 0 .. upto"""
    xs, vs = exact_posterior_fractions(z[:upto + 1], seen[:upto + 1], q, r, vv)
    return xs[-1], vs[-1]


def exact_forecast(z, seen, q, r, vv, m):
    """x_last + m v_last from the exact filtered mean at the last sighting, rounded once"""
    last = max(f for f in range(len(z)) if seen[f])
    x, v = exact_filtered(z, seen, q, r, vv, last)
    return float(x + Fraction(int(m)) * v), float(v)


# ---- 2. the kernel's statements restated, one component, with plantable defects -----------------------------------------------------------------
DEFECTS = ("q2_for_q4", "gain_without_r", "c01_c10_swapped", "class_swapped", "back_from_predicted", "forecast_from_smoothed")


def restated(z, seen, q, r, vv, defect=None, q_other=None, m=0):
    """TRAJ_UPDATE, traj_predict_cov and TRAJ_BACK statement for statement in numpy float64 for ONE component of noise q.  Returns
    xs, vs [n], and the forecast (x_last + m v_last, v_last).  defect: one of DEFECTS; `class_swapped` runs the component with
    q_other, the noise of the other class."""
    f64 = np.float64
    n = len(z)
    q = f64(q_other if defect == "class_swapped" else q)
    r, vv = f64(r), f64(vv)
    q2, q4 = f64(0.5) * q, f64(0.25) * q
    if defect == "q2_for_q4":
        q4 = q2
    X, V, XP, VP, P, PP = [None] * n, [None] * n, [None] * n, [None] * n, [None] * n, [None] * n
    x, v, pxx, pxv, pvv = f64(z[0]), f64(0.0), r, f64(0.0), vv
    X[0], V[0], P[0] = x, v, (pxx, pxv, pvv)
    last = 0
    with np.errstate(all="ignore"):
        for f in range(1, n):
            a, b = pxx + pxv, pxv + pvv
            nxx, nxv, nvv = (a + b) + q4, b + q2, pvv + q
            xp, vp = x + v, v
            if seen[f]:
                sn = nxx if defect == "gain_without_r" else nxx + r
                kx, kv = nxx / sn, nxv / sn
                pxx, pxv, pvv = nxx - kx * nxx, nxv - kx * nxv, nvv - kv * nxv
                e = f64(z[f]) - xp
                x, v = xp + kx * e, vp + kv * e
                last = f
            else:
                x, v, pxx, pxv, pvv = xp, vp, nxx, nxv, nvv
            X[f], V[f], XP[f], VP[f], P[f], PP[f] = x, v, xp, vp, (pxx, pxv, pvv), (nxx, nxv, nvv)
        xs, vs = np.zeros(n), np.zeros(n)
        xs[n - 1], vs[n - 1] = (XP[n - 1], VP[n - 1]) if (defect == "back_from_predicted" and n > 1) else (X[n - 1], V[n - 1])
        for f in range(n - 2, -1, -1):
            pxx, pxv, pvv = P[f]
            nxx, nxv, nvv = PP[f + 1]
            g00, g01, g10, g11 = pxx + pxv, pxv, pxv + pvv, pvv
            det = nxx * nvv - nxv * nxv
            C00, C01 = (g00 * nvv - g01 * nxv) / det, (g01 * nxx - g00 * nxv) / det
            C10, C11 = (g10 * nvv - g11 * nxv) / det, (g11 * nxx - g10 * nxv) / det
            if defect == "c01_c10_swapped":
                C01, C10 = C10, C01
            dx, dv = xs[f + 1] - XP[f + 1], vs[f + 1] - VP[f + 1]
            xs[f], vs[f] = X[f] + (C00 * dx + C01 * dv), V[f] + (C10 * dx + C11 * dv)
        xl, vl = X[last], V[last]
        if defect == "forecast_from_smoothed":                     # (at `last` itself the smoothed state IS the filtered one: the defect
            xl, vl = X[last], vs[max(last - 1, 0)]                 # that can occur reads the smoothed velocity of the frame before)
        fc = (xl + f64(m) * vl, vl)
    return xs, vs, fc


def error_units(z, seen, got, want):
    """max |got - want| in units of 2^-24 max|z| over the sightings; a non-finite value is inf"""
    scale = UNIT * max(abs(float(z[f])) for f in range(len(z)) if seen[f])
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.abs(got - want))) / scale


# ---- 3. the tracks of the sweep --------------------------------------------------------------------------------------------------------------
def sweep_track(n, gap, amp, seed):
    """z [n] float32-valued float64 and seen [n]: a drifting track of amplitude `amp` with jitter and ONE run of `gap` unseen frames in
    the middle (n >= gap + 2, else no gap), the last frame a sighting"""
    rng = np.random.default_rng(seed)
    f = np.arange(n)
    z = amp * (0.35 + 0.5 * f / max(n - 1, 1) + 0.1 * np.sin(0.9 * f) + 0.05 * rng.normal(size=n))
    z = z.astype(np.float32).astype(np.float64)
    seen = np.ones(n, bool)
    if gap and n >= gap + 2:
        at = 1 + (n - gap - 2) // 2
        seen[at:at + gap] = False
    return z, seen


@functools.lru_cache(maxsize=None)
def sweep_tracks():
    """[(label, z, seen)]: spans of 2, 3, 24 and 64 frames, gaps of 0, 1, 2, 8, 16 (and 40 in the 64-frame span), |z| near 1 and 1e-3"""
    out = []                                                       # (shared, never modified)
    for n, gaps in ((2, (0,)), (3, (0, 1)), (24, (0, 1, 2, 8, 16)), (64, (0, 16, 40))):
        for gap in gaps:
            for amp in (1.0, 1e-3):
                z, seen = sweep_track(n, gap, amp, 100 * n + gap)
                out.append(("n%d gap%d amp%g" % (n, gap, amp), z, seen))
    return tuple(out)


def reference_track(z, seen, q, r, vv):
    """trajectory.reference_smooth's own recursion (`_smooth_track`: the float64 restatement the device is held to, bit for bit) on one
    component: xs, vs [n] and the filtered (x, v) at the last frame.  The entry's argument checks are not in the way here."""
    z4 = lambda f: np.full(4, z[f], np.float64) if seen[f] else None
    with np.errstate(all="ignore"):
        xs, vs, (xl, vl) = trajectory._smooth_track(z4, 0, len(z) - 1, np.full(4, q, np.float64), np.float64(r), np.float64(vv))
    n = len(z)
    return np.array([xs[f][0] for f in range(n)]), np.array([vs[f][0] for f in range(n)]), (xl[0], vl[0])


FORECAST_M = 16                                                    # the forecast measured next to the sweep: m = MAX_HORIZON frames ahead


def reference_error(z, seen, q, r, vv, exact=None):
    """(position error, velocity error, forecast error at m = FORECAST_M) of `reference_track` in units, against the exact posterior.
    The track ends in a sighting, so the filtered state at `last` is the smoothed one of the last frame."""
    assert seen[-1]
    xe, ve = exact if exact is not None else exact_posterior(z, seen, q, r, vv)
    xs, vs, (xl, vl) = reference_track(z, seen, q, r, vv)
    with np.errstate(all="ignore"):
        fc = xl + np.float64(FORECAST_M) * vl
    return error_units(z, seen, xs, xe), error_units(z, seen, vs, ve), error_units(z, seen, [fc], [xe[-1] + FORECAST_M * ve[-1]])


# ---- 4. the sweep ---------------------------------------------------------------------------------------------------------------------------
Q_DECADES = tuple(range(-30, 21))                                  # q / r = 10^k
V_DECADES = (None,) + tuple(range(-20, 21))                        # velocity_var / r = 0 (None), 10^k
R_DECADES = tuple(range(-150, 151))                                # r = 2^round(k log2 10): within a factor 1.42 of 10^k, and q = (q / r) r,
R_HOME = -3                                                        # velocity_var = (v / r) r are exact products, so one exact solve serves every r
LIMITS = dict(q_over_r_min=trajectory.Q_OVER_R_MIN, q_over_r_max=trajectory.Q_OVER_R_MAX, v_over_r_max=trajectory.V_OVER_R_MAX,
              r_min=trajectory.R_MIN, r_max=trajectory.R_MAX)

INF = float("inf")
# A RECORD, not a measurement the suite repeats: regenerate it (python tests/smoother_cases.py) whenever trajectory._smooth_track changes.
# the full sweep (sweep_plan("full"): 16852 (track, q / r, v / r) points, 294052 with the decades of r), worst position / velocity error in
# units per decade: "q" over v / r <= 1e6, "v" over 1e-29 <= q / r <= 1e15 (None: velocity_var = 0), "r" over both
_SWEEP_Q = {-30: 1.8e-05, -29: 1.8e-05, -28: 4.4e-06, -27: 4.4e-06, -26: 4.4e-06, -25: 1.8e-05, -24: 4.4e-06, -23: 4.4e-06, -22: 4.4e-06, -21: 4.4e-06,
            -20: 1.8e-05, -19: 4.4e-06, -18: 4.4e-06, -17: 4.4e-06, -16: 4.4e-06, -15: 1.8e-05, -14: 4.4e-06, -13: 4.4e-06, -12: 4.4e-06, -11: 2.8e-05,
            -10: 0.00036, -9: 0.0023, -8: 0.00036, -7: 0.0023, -6: 0.00028, -5: 0.003, -4: 0.003, -3: 0.0022, -2: 0.0035, -1: 0.00082,
            0: 7e-05, 1: 6e-05, 2: 5.5e-05, 3: 0.0003, 4: 1.6e-08, 5: 1.4e-05, 6: 1.3e-08, 7: 9.9e-09, 8: 1e-08, 9: 1.1e-08,
            10: 1.4e-05, 11: 1.1e-08, 12: 9.7e-09, 13: 1.5e-08, 14: 4.3e-06, 15: 1.7e-06, 16: 1.1e-06, 17: INF, 18: INF, 19: INF,
            20: INF}
_SWEEP_V = {None: 0.00017, -20: 0.00017, -19: 9.9e-09, -18: 9.9e-09, -17: 9.9e-09, -16: 9.9e-09, -15: 9.9e-09, -14: 9.9e-09, -13: 9.5e-09, -12: 7.8e-09,
            -11: 1.2e-08, -10: 0.00017, -9: 8.1e-09, -8: 9.9e-09, -7: 7.2e-09, -6: 9.7e-09, -5: 1.1e-08, -4: 1.1e-08, -3: 1.1e-08, -2: 8.4e-09,
            -1: 1.3e-08, 0: 0.00017, 1: 5.1e-08, 2: 0.00029, 3: 3.9e-06, 4: 0.0003, 5: 0.00055, 6: 0.0035, 7: 0.06, 8: 0.38,
            9: 3.1, 10: 33, 11: 4.1e+02, 12: 3.8e+03, 13: 3.2e+04, 14: 3.7e+05, 15: 1.6e+06, 16: INF, 17: INF, 18: INF,
            19: INF, 20: INF}
# (flat between its ends: r only scales the chain; at R_HOME every pair of the box is in, elsewhere the 20 pairs around the limits)
_SWEEP_R = {k: ((0.0035 if k == R_HOME else 7e-05) if -148 < k < 136 else INF) for k in R_DECADES}
FULL_SWEEP = dict(q=_SWEEP_Q, v=_SWEEP_V, r=_SWEEP_R, forecast_inside=0.0001)      # forecast: m = FORECAST_M, worst inside the limits


def decade(k):
    return 0.0 if k is None else float("1e%d" % k)


def r_of(k):
    return 2.0 ** int(round(k * math.log2(10.0)))


def sweep_plan(level):
    """[(track index, q / r decade, v / r decade, (r decades))].  level "full": what DESIGN.md section 19 records -- the short tracks
    (spans 2 and 3) at every (q / r, v / r) pair of decades, the long ones at every q / r decade in -10 .. 3 and every fifth elsewhere
    against ten v / r columns, and every decade of r at 42 (q / r, v / r) pairs around the limits (20 of them inside), all tracks.  level "test": the part
    test_smoother_cases_host.py repeats in seconds, all of it INSIDE the limits -- the short tracks along every axis through the
    defaults and along the faces of the box, two long tracks at the defaults and the corners, the corners at both limits of r."""
    tracks = sweep_tracks()
    short = [i for i, (_, z, _) in enumerate(tracks) if len(z) <= 3]
    long_ = [i for i in range(len(tracks)) if i not in short]
    plan = []
    if level == "full":
        q_c, v_c = (-30, -29, -6, 0, 14, 15, 16), (None, -20, 2, 6, 7, 8)
        q_long = tuple(k for k in Q_DECADES if -10 <= k <= 3 or k % 5 == 0 or k in q_c)
        v_long = (None, -20, -10, 0, 2, 4, 5, 6, 7, 8)
        for i in short:
            plan += [(i, qk, vk, R_DECADES if (qk in q_c and vk in v_c) else (R_HOME,)) for qk in Q_DECADES for vk in V_DECADES]
        for i in long_:
            plan += [(i, qk, vk, R_DECADES if (qk in q_c and vk in v_c) else (R_HOME,)) for qk in q_long for vk in v_long]
        return plan
    lo, hi = int(round(math.log10(LIMITS["q_over_r_min"]))), int(round(math.log10(LIMITS["q_over_r_max"])))
    vhi = int(round(math.log10(LIMITS["v_over_r_max"])))
    rlo, rhi = int(round(math.log10(LIMITS["r_min"]))), int(round(math.log10(LIMITS["r_max"])))
    q_in = [k for k in Q_DECADES if lo <= k <= hi]
    v_in = [k for k in V_DECADES if k is None or k <= vhi]
    corners = [(qk, vk) for qk in (lo, hi) for vk in (None, vhi)]
    pairs = set()
    for vk in (None, -20, 2, vhi):
        pairs |= {(qk, vk) for qk in q_in}
    for qk in (lo, -6, -1, 0, hi):
        pairs |= {(qk, vk) for vk in v_in}
    for i in short:
        plan += [(i, qk, vk, (R_HOME, rlo, rhi) if (qk, vk) in corners else (R_HOME,))
                 for qk, vk in sorted(pairs, key=lambda a: (a[0], -99 if a[1] is None else a[1]))]
    for i in long_:
        if tracks[i][0] in ("n24 gap16 amp0.001", "n64 gap40 amp1"):
            plan += [(i, 0, 2, (R_HOME,))] + [(i, qk, vk, (R_HOME, rlo, rhi)) for qk, vk in corners]
    return plan


def sweep_job(item):
    """one entry of a plan: [(label, q / r decade, v / r decade, r decade, position, velocity, forecast error in units)]"""
    i, qk, vk, r_decades = item
    label, z, seen = sweep_tracks()[i]
    qr, vr = decade(qk), decade(vk)
    exact, out = None, []
    for rk in r_decades:
        r = r_of(rk)
        q, vv = qr * r, vr * r
        assert q / r == qr and vv / r == vr                        # exact products: the posterior mean does not depend on r
        if exact is None:
            exact = exact_posterior(z, seen, q, r, vv)
        out.append((label, qk, vk, rk) + reference_error(z, seen, q, r, vv, exact))
    return out


def sweep_summary(rows, q_range=(-29, 15), v_max=6):
    """{axis: {decade: worst position / velocity error over the tracks}}: per q / r decade over v / r <= 10^v_max, per v / r decade
    over q / r within q_range (both with r at R_HOME), per r decade over both, and the forecast's worst at m = FORECAST_M over the same
    rows as "r" and at R_HOME ("forecast")"""
    worst = {"q": {}, "v": {}, "r": {}, "forecast": {}}
    fix = lambda e: float("inf") if e != e else e
    for label, qk, vk, rk, ep, ev, ef in rows:
        e, q_in, v_in = fix(max(ep, ev)), q_range[0] <= qk <= q_range[1], vk is None or vk <= v_max
        if rk == R_HOME:
            if v_in:
                worst["q"][qk] = max(worst["q"].get(qk, 0.0), e)
            if q_in:
                worst["v"][vk] = max(worst["v"].get(vk, 0.0), e)
        if q_in and v_in:
            worst["r"][rk] = max(worst["r"].get(rk, 0.0), e)
            worst["forecast"][rk] = max(worst["forecast"].get(rk, 0.0), fix(ef))
    return worst


# ---- 5. windows: every operand a window of a NaN / -77777 parent, every output a primed window of a sentinel parent --------------------------
IN_FILL = {"f": float("nan"), "i": -77777, "b": -77}               # float / int32 / int8 parents of operands
OUT_FILL = {"f": -12345.5, "i": -55555, "b": 0x5A}                 # parents of outputs and of in-place state
PRIMER = {"f": float("nan"), "i": -999, "b": 99}                   # what an output holds before the launch


def _kind(dtype):
    dtype = np.dtype(dtype)
    return "f" if dtype.kind == "f" else ("b" if dtype.itemsize == 1 else "i")


class Window:
    """a contiguous window of a flat numpy parent: 16 (+ off) elements in front, 16 behind.  kind "in": `values` inside a parent of
    IN_FILL; "out": PRIMER inside OUT_FILL; "state": `values` inside OUT_FILL.  off: elements past the 16-element boundary (float32:
    off = 1 is 4 bytes past a 16-byte boundary)"""

    def __init__(self, kind, values=None, shape=None, dtype=None, off=0):
        if values is not None:
            values = np.ascontiguousarray(values)
            shape, dtype = values.shape, values.dtype
        self.kind, self.shape, self.dtype, self.lead = kind, tuple(shape), np.dtype(dtype), 16 + int(off)
        self.n = int(np.prod(self.shape))
        k = _kind(dtype)
        fill = IN_FILL[k] if kind == "in" else OUT_FILL[k]
        self.parent = np.full(self.lead + self.n + 16, fill, self.dtype if k == "f" else np.int64).astype(self.dtype)
        self.parent[self.lead:self.lead + self.n] = PRIMER[k] if kind == "out" else values.reshape(-1)
        self.byte_offset = self.lead * self.dtype.itemsize

    def inside(self, parent):
        return np.asarray(parent)[self.lead:self.lead + self.n].reshape(self.shape)

    def outside_changed(self, parent):
        """the number of bytes outside the window (kind "in": anywhere) that differ from what the parent held before the launch"""
        a, b = np.asarray(parent).view(np.uint8), self.parent.view(np.uint8)
        diff = a != b
        if self.kind != "in":
            diff[self.byte_offset:self.byte_offset + self.n * self.dtype.itemsize] = False
        return int(diff.sum())

    def unwritten(self, parent):
        """kind "out": the number of elements that still hold the primer"""
        v, k = self.inside(parent).reshape(-1), _kind(self.dtype)
        return int(np.isnan(v).sum()) if k == "f" else int((v == PRIMER[k]).sum())


# ---- 6. planted tracker tables ----------------------------------------------------------------------------------------------------------------
IMG = (50, 50)


def track_values(n, seed, amp=1.0):
    """z [n, 4] float32 = [sx, tx, sy, ty] within amp [0.4, 1.0]: drift, a slow wave and jitter per component; sy = sx (one exact solve
    less per track).  Every smoothed value stays within a factor 64 of max|z| (test_smoother_cases_host.py asserts it and says why)"""
    rng = np.random.default_rng(seed)
    f = np.arange(n)[:, None]
    slope = np.array([0.05, 0.3, 0.05, -0.3]) * rng.uniform(0.5, 1.0, 4)
    z = 0.7 + slope * (f / max(n - 1, 1) - 0.5) + 0.08 * np.sin(0.9 * f + np.arange(4)) + 0.03 * rng.normal(size=(n, 4))
    z[:, 2] = z[:, 0]
    return (amp * z).astype(np.float32)


def track(first, pattern, seed, amp=1.0):
    """a track born in frame `first` with the sightings of `pattern` (a string of 1 / 0, first and last 1)"""
    seen = np.array([c == "1" for c in pattern])
    assert seen[0] and seen[-1]
    return dict(first=int(first), seen=seen, z=track_values(len(seen), seed, amp))


def planted_case(F, T, max_age, seqs, A=4, G=4, seed=0):
    """the tables a tracker would have written for `seqs` (per sequence the tracks in id order): where [T, R, 4], n [R], track_id [T, R],
    num_tracks [S], track_first / track_last [S, F T], and provider rows what / glimpse / score for the fills.  The sightings of a frame
    take its slots rotated by the frame index; the slots at and beyond n hold NaN and the id of a live track: they are never read."""
    S, R = len(seqs), len(seqs) * F
    rng = np.random.default_rng(seed)
    where, ids, n = np.full((T, R, 4), np.nan, np.float32), np.zeros((T, R), np.int32), np.zeros(R, np.int32)
    first, last = np.full((S, F * T), -1, np.int32), np.full((S, F * T), -1, np.int32)
    per_row = [[] for _ in range(R)]
    for s, tracks in enumerate(seqs):
        for i, t in enumerate(tracks):
            first[s, i], last[s, i] = t["first"], t["first"] + len(t["seen"]) - 1
            assert last[s, i] < F
            for k in np.nonzero(t["seen"])[0]:
                per_row[s * F + t["first"] + k].append((i, t["z"][k]))
    for r, objs in enumerate(per_row):
        assert len(objs) <= T, "frame %d holds %d sightings, T = %d" % (r, len(objs), T)
        objs = objs[r % max(len(objs), 1):] + objs[:r % max(len(objs), 1)]
        for j, (i, z) in enumerate(objs):
            where[j, r], ids[j, r] = z, i
        n[r] = len(objs)
    case = dict(where=where, n=n, track_id=ids, num_tracks=np.array([len(t) for t in seqs], np.int32), track_first=first, track_last=last,
                what=rng.normal(size=(T, R, A)).astype(np.float32), glimpse=rng.uniform(size=(T, R, G)).astype(np.float32),
                score=rng.uniform(size=(T, R)).astype(np.float32), T=T, R=R, F=F, S=S, max_age=max_age, img=IMG, A=A, G=G, seqs=seqs)
    return case


def at_limit(ratio, r, upper):
    """the LAST float64 x whose float64 quotient x / r is on the inner side of `ratio`, the limit included (the entry compares the
    quotient): from ratio * r outwards until the quotient crosses the limit, then back inwards until it does not"""
    out, back = (np.inf, 0.0) if upper else (0.0, np.inf)
    crossed = (lambda x: x / r > ratio) if upper else (lambda x: x / r < ratio)
    x = np.float64(ratio * r)
    while not crossed(x):
        x = np.nextafter(x, out)
    while crossed(x):
        x = np.nextafter(x, back)
    return float(x)


def noise_rows():
    """{name: noise kwargs}: the defaults, each limit of the measured box alone, and all together at velocity_var = 0 and at
    V_OVER_R_MAX r; the shift and the scale class at opposite limits of q / r"""
    D, lim = trajectory.DEFAULTS, LIMITS
    r0 = D["measurement_noise"]
    qhi, qlo = (lambda r: at_limit(lim["q_over_r_max"], r, True)), (lambda r: at_limit(lim["q_over_r_min"], r, False))
    vhi = lambda r: at_limit(lim["v_over_r_max"], r, True)
    rows = {"defaults": dict(D),
            "q_max": dict(D, process_noise=(qhi(r0), 0.25 * r0)),
            "q_min": dict(D, process_noise=(0.25 * r0, qlo(r0))),
            "v_max": dict(D, velocity_var=vhi(r0)),
            "v_zero": dict(D, velocity_var=0.0),
            "r_min": dict(process_noise=(0.25 * lim["r_min"],) * 2, measurement_noise=lim["r_min"], velocity_var=100.0 * lim["r_min"]),
            "r_max": dict(process_noise=(0.25 * lim["r_max"],) * 2, measurement_noise=lim["r_max"], velocity_var=100.0 * lim["r_max"])}
    for rn in ("r_min", "r_max"):
        r = lim[rn]
        rows["all_%s_v_zero" % rn] = dict(process_noise=(qhi(r), qlo(r)), measurement_noise=r, velocity_var=0.0)
        rows["all_%s_v_max" % rn] = dict(process_noise=(qhi(r), qlo(r)), measurement_noise=r, velocity_var=vhi(r))
    rows["all_swapped"] = dict(process_noise=(qlo(lim["r_min"]), qhi(lim["r_min"])), measurement_noise=lim["r_min"], velocity_var=vhi(lim["r_min"]))
    return rows


def outside_rows():
    """{name: noise kwargs} just outside each limit, and the settings of the issue's table that lie outside: all refused"""
    D, lim = trajectory.DEFAULTS, LIMITS
    r0, up, down = D["measurement_noise"], (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, 0.0)))
    return {"q_shift_above": dict(D, process_noise=(up(at_limit(lim["q_over_r_max"], r0, True)), 1e-4)),
            "q_scale_above": dict(D, process_noise=(1e-4, up(at_limit(lim["q_over_r_max"], r0, True)))),
            "q_shift_below": dict(D, process_noise=(down(at_limit(lim["q_over_r_min"], r0, False)), 1e-4)),
            "q_scale_below": dict(D, process_noise=(1e-4, down(at_limit(lim["q_over_r_min"], r0, False)))),
            "v_above": dict(D, velocity_var=up(at_limit(lim["v_over_r_max"], r0, True))),
            "r_below": dict(process_noise=(0.25 * lim["r_min"],) * 2, measurement_noise=down(lim["r_min"]), velocity_var=0.0),
            "r_above": dict(process_noise=(0.25 * lim["r_max"],) * 2, measurement_noise=up(lim["r_max"]), velocity_var=0.0),
            "issue_vv_1e6": dict(D, velocity_var=1e6), "issue_vv_1e8": dict(D, velocity_var=1e8), "issue_vv_1e10": dict(D, velocity_var=1e10),
            "issue_vv_1e12": dict(D, velocity_var=1e12), "issue_vv_1e14": dict(D, velocity_var=1e14),
            "issue_r_3e-17": dict(process_noise=(1.0, 1.0), measurement_noise=3e-17, velocity_var=0.0),
            "issue_r_1e-17": dict(process_noise=(1.0, 1.0), measurement_noise=1e-17, velocity_var=1e-20),
            "issue_1e-300": dict(process_noise=(1e-300, 1e-300), measurement_noise=1e-300, velocity_var=0.0)}


def _gap_case(max_age):
    """one sequence, T = 2: a track with a gap of exactly max_age frames, and one that misses max_age + 1 frames, dies and is reborn
    under a new id"""
    g = max_age
    a = "11" + "0" * g + "11" + "0" * g + "1"
    F = len(a) + 1
    b1, b2_first = "11", 2 + g + 1
    b2 = "1" * (F - b2_first)
    return planted_case(F, 2, max_age, [[track(0, a + "1", 11 + g), track(0, b1, 12 + g), track(b2_first, b2, 13 + g)]], seed=g)


def _lanes_case():
    """T = 5, F = 40, max_age = 1: 139 ids, three passes of lanes.  Id 0 spans every frame and id 69 the frames from 17 on (both with
    dropouts); every other id is one sighting.  The ids of the third pass (128 ..) overlap id 0 (first chunk of ids) and id 69 (second)"""
    F, tracks, by_first = 40, [], {}
    long_a = track(0, "1101" + "1" * 20 + "0" + "1" * 15, 21)
    long_b = track(17, "11011" + "1" * 10 + "01" + "1" * 6, 22)
    for f in range(F):
        born = ([long_a] if f == 0 else []) + ([long_b] if f == 17 else [])
        churn = 4 if f < 17 else 3
        born += [track(f, "1", 1000 + 10 * f + k) for k in range(churn)]
        tracks += born
    case = planted_case(F, 5, 1, [tracks], seed=3)
    assert tracks[0] is long_a and tracks[69] is long_b and len(tracks) > 128
    return case


def _overflow_case():
    """T = 32, F = 4, max_age = 1, C = 32: 33 tracks span frame 1 (id 0 coasts over it, ids 1 .. 31 are sighted, id 32 is born), ids
    16 .. 31 end there: id 32 has row 32 >= C in frame 1 and row 16 in frames 2 and 3"""
    tracks = [track(0, "1011", 300)] + [track(0, "1111", 300 + i) for i in range(1, 16)] + [track(0, "11", 300 + i) for i in range(16, 32)]
    tracks.append(track(1, "111", 332))
    return planted_case(4, 32, 1, [tracks], seed=4)


def _cap_case():
    """a table no tracker writes: 33 lower ids overlap id 33 (the device keeps the 32 lowest); the 33rd (id 32) ends before any frame
    in which id 33 has a row below C, so the count of the 32 lowest is the count of all"""
    tracks = [track(0, "101", 400 + i) for i in range(16)] + [track(0, "11", 400 + i) for i in range(16, 32)]
    tracks += [track(1, "1", 432), track(1, "11", 433)]
    return planted_case(3, 32, 1, [tracks], seed=5)


ONE_SHOT = {                                                       # name -> (case builder, horizon, noise rows)
    "mixed": (lambda: planted_case(8, 3, 2, [[track(0, "11111111", 1), track(1, "1010011", 2), track(6, "11", 3)],
                                              [track(0, "11011", 4), track(2, "111001", 5, amp=1e-3)]], seed=1), 3, "all"),
    "span64": (lambda: planted_case(64, 1, 40, [[track(0, "1111" + "0" * 16 + "11" + "0" * 40 + "11", 6)]], seed=2), 3,
               ("defaults", "v_max")),
    "gap0": (lambda: _gap_case(0), 2, ("defaults",)), "gap1": (lambda: _gap_case(1), 2, ("defaults",)),
    "gap2": (lambda: _gap_case(2), 2, ("defaults",)), "gap8": (lambda: _gap_case(8), 2, ("defaults",)),
    "lanes3": (_lanes_case, 2, ("defaults",)),
    "overflow": (_overflow_case, 2, ("defaults", "all_r_max_v_zero")),
}
_CASES = {}


def one_shot_case(name):
    if name not in _CASES:
        _CASES[name] = ONE_SHOT[name][0]()
    return _CASES[name]


def one_shot_rows():
    """[(case name, noise row name)]"""
    return [(name, row) for name, (_, _, rows) in ONE_SHOT.items() for row in (list(noise_rows()) if rows == "all" else rows)]


# ---- 7. the exact tables of a case and the check of a result against them ----------------------------------------------------------------------
_EXACT = {}


def _exact_cached(z, seen, q, r, vv):
    """exact_posterior_fractions, shared: the posterior mean depends on q / r and velocity_var / r alone"""
    key = (z.tobytes(), seen.tobytes(), Fraction(q) / Fraction(r), Fraction(vv) / Fraction(r))
    if key not in _EXACT:
        _EXACT[key] = exact_posterior_fractions(z, seen, q, r, vv)
    return _EXACT[key]


def exact_track(t, noise, upto=None):
    """the exact smoothed (xs, vs) [n, 4] float64 of a planted track given its frames up to index `upto` (None: all), cut after the
    last sighting at or before it; None where the track has no sighting there.  Components [sx, tx, sy, ty]: the odd ones are shifts"""
    seen = t["seen"] if upto is None else t["seen"][:upto + 1]
    n = int(np.nonzero(seen)[0][-1]) + 1
    q_shift, q_scale = noise["process_noise"]
    xs, vs = np.zeros((n, 4)), np.zeros((n, 4))
    for c in range(4):
        fx, fv = _exact_cached(t["z"][:n, c].astype(np.float64), t["seen"][:n], q_shift if c % 2 else q_scale, noise["measurement_noise"],
                               noise["velocity_var"])
        xs[:, c], vs[:, c] = [float(v) for v in fx], [float(v) for v in fv]
    return xs, vs


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def column_ratios(t, where, velocity, xe, ve, img=IMG):
    """(position ratio, velocity ratio) of one table row against the exact (x, v) [4]: |where - fp32(x)| / ulp and |velocity -
    fp32(pixels of v)| / (one unit of 2^-24 max|z| in pixels per frame)"""
    H, W = img
    zmax = float(np.abs(t["z"][t["seen"]]).max())
    want = xe.astype(np.float32)
    rp = float(np.max(np.abs(where.astype(np.float64) - want.astype(np.float64)) / ulp32(want)))
    vel = np.array([(W * ve[1]) * 0.5, (H * ve[3]) * 0.5]).astype(np.float32)
    unit = UNIT * zmax * np.array([W, H]) * 0.5
    rv = float(np.max(np.abs(velocity.astype(np.float64) - vel.astype(np.float64)) / unit))
    bad = not (np.isfinite(where).all() and np.isfinite(velocity).all())
    return (float("inf"), float("inf")) if bad else (rp, rv)


def check_exact(case, out, horizon, noise):
    """a result of air_track_smooth (the device's or reference_smooth's) against the exact posterior: every row of the completed table
    of every track, and the forecast rows.  Returns (worst position ratio, worst velocity ratio, rows checked): each must be <= 1"""
    F, S = case["F"], case["S"]
    worst_p, worst_v, checked = 0.0, 0.0, 0
    for s, tracks in enumerate(case["seqs"]):
        for i, t in enumerate(tracks):
            xs, vs = exact_track(t, noise)
            for k in range(len(t["seen"])):
                col = s * F + t["first"] + k
                row = np.nonzero(out["sm_id"][:, col] == i)[0]
                if len(row) == 0:
                    continue                                       # (a row at or beyond C: dropped)
                rp, rv = column_ratios(t, out["sm_where"][row[0], col], out["sm_velocity"][row[0], col], xs[k], vs[k], case["img"])
                worst_p, worst_v, checked = max(worst_p, rp), max(worst_v, rv), checked + 1
            la = t["first"] + len(t["seen"]) - 1
            if horizon and F - 1 - la <= case["max_age"]:
                for k in range(1, horizon + 1):
                    col = s * horizon + k - 1
                    row = np.nonzero(out["fc_id"][:, col] == i)[0]
                    if len(row) == 0:
                        continue
                    m = F - 1 - la + k
                    xe = np.array([xs[-1, 0], xs[-1, 1] + m * vs[-1, 1], xs[-1, 2], xs[-1, 3] + m * vs[-1, 3]])
                    rp, rv = column_ratios(t, out["fc_where"][row[0], col], out["fc_velocity"][row[0], col], xe, vs[-1], case["img"])
                    worst_p, worst_v, checked = max(worst_p, rp), max(worst_v, rv), checked + 1
    return worst_p, worst_v, checked


def reference(case, horizon, noise, fills=True):
    rows = dict(what=case["what"], glimpse=case["glimpse"], score=case["score"]) if fills else {}
    return trajectory.reference_smooth(case["where"], case["n"], case["track_id"], case["num_tracks"], case["track_first"],
                                       case["track_last"], case["F"], case["max_age"], case["img"], horizon, **noise, **rows)


# ---- 8. streams: the same planted sequences in chunks ----------------------------------------------------------------------------------------
def stream_sequences():
    """S = 2, 12 frames, T = 3, max_age = 2 (every gap is at most max_age, so the stream's own table holds the planted tracks; the
    track that dies is reborn under a new id)"""
    return planted_case(12, 3, 2, [[track(0, "110111001111", 51), track(1, "1011", 52), track(8, "1101", 53)],
                                   [track(0, "1" * 12, 54), track(3, "100101", 55, amp=1e-3)]], A=4, G=9, seed=6)


def ragged_valids(S, F, total):
    """raw valid [S] per chunk until every sequence has given its `total` frames: F, 0, less than F, negative, above F in turn (the
    kernel clips to 0 .. F); a sequence never gets more than it has left"""
    pattern, left, out, k = (F, 0, F - 1, -2, F + 3), [total] * S, [], 0
    while any(left):
        v = []
        for s in range(S):
            raw = pattern[(k + 2 * s) % len(pattern)]
            take = min(max(raw, 0), F)
            if take > left[s]:
                raw = take = left[s]
            left[s] -= take
            v.append(raw)
        out.append(np.array(v, np.int32))
        k += 1
    return out


def stream_chunks(case, F, valids):
    """the chunks of a stream over a planted case: sequence s holds its next clip(valid[s], 0, F) frames, behind them NaN rows with
    ids and counts of 99 that are never read.  Each chunk carries `taken` [S] and `seen_before` [S]"""
    T, S, Ft = case["T"], case["S"], case["F"]
    at, chunks = np.zeros(S, np.int64), []
    for v in valids:
        R = S * F
        c = {k: np.full((T, R) + case[k].shape[2:], np.nan, np.float32) for k in ("where", "what", "glimpse", "score")}
        c["n"], c["track_id"] = np.full(R, 99, np.int32), np.full((T, R), 99, np.int32)
        take = np.clip(v, 0, F).astype(np.int64)
        for s in range(S):
            src, dst = slice(s * Ft + at[s], s * Ft + at[s] + take[s]), slice(s * F, s * F + take[s])
            for k in ("where", "what", "glimpse", "score", "track_id"):
                c[k][:, dst] = case[k][:, src]
            c["n"][dst] = case["n"][src]
        c.update(valid=np.asarray(v, np.int32), taken=take, seen_before=at.copy(), F=F)
        chunks.append(c)
        at = at + take
    assert (at == Ft).all()
    return chunks


STREAMS = [                                                        # (chunk frames F, lag L, horizon Hz, noise row): every noise row
    (1, 2, 0, "defaults"), (2, 4, 3, "defaults"), (5, 16, 16, "defaults"), (2, 2, 3, "all_r_min_v_max"), (5, 4, 3, "all_r_max_v_zero"),
    (1, 16, 3, "q_max"), (2, 4, 0, "v_max"), (5, 2, 3, "q_min"), (1, 4, 3, "all_r_min_v_zero"), (2, 16, 3, "all_r_max_v_max"),
    (5, 2, 0, "all_swapped"), (1, 2, 3, "v_zero"), (2, 4, 16, "r_min"), (5, 16, 3, "r_max")]
assert {row for _, _, _, row in STREAMS} == set(noise_rows())


def stream_reference(case, F, lag, horizon, noise, chunks):
    """[(outputs, state after, tail)] per chunk: reference_smooth_stream and reference_smooth_tail"""
    state, res = None, []
    for c in chunks:
        out, state = trajectory.reference_smooth_stream(state, c["where"], c["n"], c["track_id"], F, c["valid"], lag, case["max_age"],
                                                        case["img"], horizon, what=c["what"], glimpse=c["glimpse"], score=c["score"], **noise)
        res.append((out, state, trajectory.reference_smooth_tail(state, lag, case["max_age"], case["img"])))
    return res


def _stream_column_ratios(case, s, g, hi, table, pre, col, noise, must):
    """column `col` of a table that holds global frame g of sequence s smoothed with the frames up to hi, against the exact FIXED-LAG
    posterior: exact_posterior restricted to the frames <= hi.  must: the ids are asserted to be exactly the planted tracks that
    span g with a sighting in g .. hi"""
    worst_p, worst_v, n = 0.0, 0.0, 0
    want_ids = []
    for i, t in enumerate(case["seqs"][s]):
        k, upto = g - t["first"], min(hi - t["first"], len(t["seen"]) - 1)
        if k < 0 or k > upto or not t["seen"][k:upto + 1].any():
            continue
        want_ids.append(i)
        row = np.nonzero(table[pre + "id"][:, col] == i)[0]
        assert len(row) == 1, (s, g, hi, i)
        xs, vs = exact_track(t, noise, upto)
        rp, rv = column_ratios(t, table[pre + "where"][row[0], col], table[pre + "velocity"][row[0], col], xs[k], vs[k], case["img"])
        worst_p, worst_v, n = max(worst_p, rp), max(worst_v, rv), n + 1
    if must:
        assert sorted(int(v) for v in table[pre + "id"][:, col] if v >= 0) == want_ids, (s, g, hi)
    return worst_p, worst_v, n


def check_stream_exact(case, F, lag, horizon, noise, chunk, out, tail):
    """one push's emitted columns, its forecast and the tail behind it against the exact posterior; (worst position ratio, worst
    velocity ratio, rows checked)"""
    S = case["S"]
    wp, wv, n = 0.0, 0.0, 0
    for s in range(S):
        b = int(chunk["seen_before"][s] + chunk["taken"][s])
        for e in range(int(out["num_emitted"][s])):
            g = int(out["emit_frame"][s, e])
            a = _stream_column_ratios(case, s, g, g + lag, out, "sm_", s * F + e, noise, True)
            wp, wv, n = max(wp, a[0]), max(wv, a[1]), n + a[2]
        for j in range(lag if tail is not None else 0):
            g = int(tail["tail_frame"][s, j])
            if g >= 0:
                a = _stream_column_ratios(case, s, g, b - 1, tail, "tl_", s * lag + j, noise, True)
                wp, wv, n = max(wp, a[0]), max(wv, a[1]), n + a[2]
        for i, t in enumerate(case["seqs"][s] if horizon and b else []):
            upto = min(b - 1 - t["first"], len(t["seen"]) - 1)
            if upto < 0:
                continue
            lf = t["first"] + int(np.nonzero(t["seen"][:upto + 1])[0][-1])
            row = np.nonzero(out["fc_id"][:, s * horizon] == i)[0]
            assert (len(row) == 1) == (b - 1 - lf <= case["max_age"]), (s, i, b, lf)
            if len(row) == 0:
                continue
            xs, vs = exact_track(t, noise, upto)
            for k in range(1, horizon + 1):
                m = b - 1 - lf + k
                xe = np.array([xs[-1, 0], xs[-1, 1] + m * vs[-1, 1], xs[-1, 2], xs[-1, 3] + m * vs[-1, 3]])
                col = s * horizon + k - 1
                rp, rv = column_ratios(t, out["fc_where"][row[0], col], out["fc_velocity"][row[0], col], xe, vs[-1], case["img"])
                wp, wv, n = max(wp, rp), max(wv, rv), n + 1
    return wp, wv, n


if __name__ == "__main__":                                         # the full sweep, as DESIGN.md section 19 records it (minutes)
    import multiprocessing
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        rows = [r for res in pool.imap_unordered(sweep_job, sweep_plan("full"), chunksize=4) for r in res]
    for axis, table in sweep_summary(rows).items():
        if axis:
            print(axis, " ".join("%s:%.2g" % (k, table[k]) for k in sorted(table, key=lambda k: -999 if k is None else k)))


# ---- 9. the size guards of the six entries: the products that index with 32 bits -----------------------------------------------------------------
# {entry: [(what the row reaches, the integer arguments to change, status)]}.  A refused call touches no table, so the shapes cost nothing.
# A row marked "control" lies just inside its guard and is refused by a LATER check with another status (a workspace of 0 bytes, a pointer
# 2 bytes off), never launched.  Dead, and so without a row: air_track_smooth_tail's C S max(L, 1) <= INT_MAX / 4 -- the state check before
# it leaves S D <= 2396745 and the same statement asks D >= L + max_age, so C S L <= 32 * 2396745 < INT_MAX / 4; and S F T <= INT_MAX of
# both smooth entries with T = 1, where R = S F is an int already.
INT_MAX = 2 ** 31 - 1
STATE_MAX_SD = INT_MAX // (28 * 32)                                # air_track_smooth_stream_state_bytes: S D beyond this gives 0
SIZE_GUARDS = {
    "smooth": [("S F T > INT_MAX", dict(T=32, S=2 ** 27, F=1, R=2 ** 27, C=32, Hz=0, max_age=0), -2),
               ("C R > INT_MAX / 4", dict(T=3, S=59652324, F=1, R=59652324, C=9, Hz=0, max_age=2), -2),
               ("control: C R = INT_MAX / 4 - 4, then the workspace", dict(T=3, S=59652323, F=1, R=59652323, C=9, Hz=0, max_age=2, ws_bytes=0), -4)],
    "fill": [("C N > INT_MAX", dict(T=1, F=1, R=67108864, C=32, N=67108864, per_seq=1), -2),
             ("T R > INT_MAX", dict(T=32, F=1, R=67108864, C=1, N=67108864, per_seq=1), -2),
             ("control: C N = INT_MAX - 31, then the alignment", dict(T=1, F=1, R=67108863, C=32, N=67108863, per_seq=1, misalign="what"), -3)],
    "stash": [("T R > INT_MAX", dict(T=32, S=67108864, F=1, R=67108864, D=1), -2),
              ("S D T > INT_MAX", dict(T=32, S=1000, F=1, R=1000, D=70000000), -2),
              ("control: T R = INT_MAX - 31, then the alignment", dict(T=32, S=67108863, F=1, R=67108863, D=1, misalign="what"), -3)],
    "fill_stream": [("C N > INT_MAX", dict(T=1, S=67108864, D=1, C=32, N=67108864, per_seq=1), -2),
                    ("S D T > INT_MAX", dict(T=32, S=1000, D=70000000, C=1, N=1000, per_seq=1), -2),
                    ("control: C N = INT_MAX - 31, then the alignment", dict(T=1, S=67108863, D=1, C=32, N=67108863, per_seq=1,
                                                                           misalign="ring_what"), -3)],
    "stream": [("S F T > INT_MAX", dict(T=32, S=2 ** 27, F=1, R=2 ** 27, C=32, L=0, Hz=0, D=1, max_age=0, state_bytes=1 << 60), -2),
               ("the state of S D frames has no size", dict(T=3, S=3000000, F=1, R=3000000, C=9, L=2, Hz=0, D=5, max_age=2, state_bytes=1 << 60), -2),
               ("F T > 32767", dict(T=32, S=1, F=1024, R=1024, C=32, L=1, Hz=0, D=8, max_age=1, state_bytes=1 << 60), -2),
               ("C R > INT_MAX / 4", dict(T=2, S=2000000, F=300, R=600000000, C=32, L=15, Hz=0, D=1, max_age=15, state_bytes=1 << 60), -2)],
}
