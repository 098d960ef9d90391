"""Trajectories behind the sequence tracker on the device: smoothed, gap-filled and extrapolated tracks, and predicted frames.

track.SequenceTracker gives the objects of a sequence identities; this module turns an identity into a trajectory.  Per track and per
`where` component [sx, tx, sy, ty] a constant-rate Kalman filter runs forward over the frames the track spans and a Rauch-Tung-Striebel
pass (means only) runs back, so that every frame's estimate uses the past and the future of the track; a frame the track coasted over
(max_age >= 1) gets a FILLED row; and the tracks still live after the last frame are extrapolated `horizon` frames ahead and rendered
with the decoded glimpse of their last sighting: the predicted frames.  No network evaluation: the glimpse depends on `what` alone.

The rule (air_track_smooth; include/air_hip.h states the same, `reference_smooth` restates it in numpy float64).  Float64 from the widened
fp32 values, only + - * /, in this order.  State (x, v), covariance (Pxx, Pxv, Pvv), dt = 1 frame; q = q_shift for tx, ty and q_scale
for sx, sy; q4 = 0.25 q, q2 = 0.5 q; r the measurement noise.
  start    at the first sighting z:  x = z, v = 0, Pxx = r, Pxv = 0, Pvv = velocity_var;
  predict  every frame up to the last sighting:  a = Pxx + Pxv, b = Pxv + Pvv, x- = x + v, v- = v, Pxx- = (a + b) + q4,
           Pxv- = b + q2, Pvv- = Pvv + q;
  update   only in a frame with a sighting z:  s = Pxx- + r, kx = Pxx- / s, kv = Pxv- / s, e = z - x-, x = x- + kx e, v = v- + kv e,
           Pxx = Pxx- - kx Pxx-, Pxv = Pxv- - kx Pxv-, Pvv = Pvv- - kv Pxv-;  a coasted frame keeps the predicted state;
  back     f = last - 1 down to first, xs[last] = x, vs[last] = v:  g00 = Pxx + Pxv, g01 = Pxv, g10 = Pxv + Pvv, g11 = Pvv (filtered,
           frame f), det = Pxx- Pvv- - Pxv- Pxv- (predicted, frame f + 1), C00 = (g00 Pvv- - g01 Pxv-) / det, C01 = (g01 Pxx- - g00
           Pxv-) / det, C10 = (g10 Pvv- - g11 Pxv-) / det, C11 = (g11 Pxx- - g10 Pxv-) / det, dx = xs[f+1] - x-[f+1], dv = vs[f+1] -
           v-[f+1], xs[f] = x + (C00 dx + C01 dv), vs[f] = v + (C10 dx + C11 dv).
Two exact consequences: a track with one sighting returns its `where` bits, and a track whose sightings all carry one value returns
that value bit for bit with v = 0.
The noise terms must lie in THE SUPPORTED DOMAIN (Q_OVER_R_MIN .. R_MAX below): inside it the rule gives the posterior mean of the
model to well under one float32 rounding of an output (measured against an exact solve: tests/smoother_cases.py);
outside it the differences P- - k P- and the quotients by det lose digits and then turn NaN, so `check_arguments` raises and the
entries return AIR_E_SHAPE (the numpy restatements alone still run there: the domain was measured with them).  A user who does not know the velocity writes velocity_var = V_OVER_R_MAX * measurement_noise.

The completed table has C = min(32, T (max_age + 1)) rows per frame: in frame f the tracks with first <= f <= last take rows
0 .. n_f - 1 in ascending id (sm_where, sm_boxes, sm_id, sm_state, sm_src_frame, sm_src_slot, sm_velocity, sm_count, sm_counts).  The
forecast table [C, S Hz] holds, for k = 1 .. Hz, the tracks with F - 1 - last <= max_age in ascending id: with m = F - 1 - last + k,
tx' = x + m v from the filtered state at `last` (ty' alike), the scales held -- a rate on a scale can cross zero.

`TrajectorySmoother` owns no engine: it binds to a track.SequenceTracker, only reads that tracker's and its provider's buffers, and
runs, on the same engine stream, ONE hipGraph after `capture()` whatever F and the horizon are:

  air_track_smooth   the rule above, both tables;
  air_track_fill     what / glimpse / score of the rows of both tables: bit copies of the source sighting's rows;
  air_parse_objects (given counts), air_tile_relabel, air_parse_render   the unchanged read-out kernels at C rows on the R completed
                     frames and on the S Hz forecast columns: boxes, the object table (obj_step = the track id), a reconstruction and
                     an owner map per completed frame, and the predicted frames [S, Hz, H, W].

`smoother.completed` exposes the provider surface (what, where, glimpse, boxes, score, presence, num_objects, owner, T = C, R, engine),
so a score.ParseScorer binds to the completed frames unchanged; the smoother's own `score(gt_boxes, ...)` is the unchanged
air_track_score with T := C on the completed table (one object cannot carry both a `score` tensor and a `score` method).

The defaults of process_noise, measurement_noise and velocity_var are provisional: UNMEASURED on a trained model (profiles/trajectory.txt
says what was measured).  `TrajectoryNoiseFitter` (NOISE FIT below) fits them to a model's own tracks by maximum likelihood, without
ground truth.  The association itself can run this rule's forward filter: track.SequenceTracker(motion=...) matches every track against
the forecast row of its filtered state (air_track_associate_motion; track.py states it under MOTION), with these noise terms, and its
pred_where is this module's fc_where (horizon 1) on the tracker's own output truncated before the frame, bit for bit; with motion_gate=
the pairs are gated by sum e^2 / s over this filter's innovation e and its variance s (track.py: THE GATE), the quantities NOISE FIT's
likelihood is made of.  Out of scope:
smoothed covariances, feeding the SMOOTHED (non-causal) rows back into the association, rates on scales in the forecast, a learned
motion prior, particle providers (refused by the tracker, in its wording).

STREAMS (`StreamSmoother` behind a track.StreamTracker; air_track_smooth_stream, `reference_smooth_stream` restates a chunk in numpy).
The rule above, unchanged, with a LAG L, max_age <= L <= MAX_LAG = 16: the forward filter is causal, and the backward pass over a
bounded window is FIXED-LAG smoothing -- the estimate of global frame g that uses the sightings up to g + L is final once frame g + L
has been seen, and it is exactly what the rule gives on the sequence truncated after frame g + L.  L >= max_age makes "does the track
span g" final by then: a track that coasts at g without a sighting in g + 1 .. g + L is retired.  A push that takes frames_seen[s]
from a to b:
  emitted   the global frames max(0, a - L) <= g < max(0, b - L), once each, ascending, at most valid[s] of them: the tracks with a
            sighting at or before g and a sighting in g .. g + L in ascending id, the backward pass run from the last sighting at or
            before g + L down to g; src_frame is a GLOBAL frame.  TRUNCATION IDENTITY: bit for bit column g of `reference_smooth` on
            the first g + L + 1 frames of the concatenation of the sequence's valid frames -- hence CHUNK INVARIANCE: any chunking,
            ragged valid and valid = 0 included, gives frame g the same bits;
  forecast  every push, no lag: bit for bit the forecast table of `reference_smooth` on the first b frames (the live tracks from the
            filtered state at `last`, m = b - 1 - last + k); valid = 0 gives it again, a sequence that has seen nothing an empty one;
  tail      on request and read-only: the frames max(0, b - L) .. b - 1, not final yet, smoothed with what is known -- the last
            columns of `reference_smooth` on the first b frames; at the end of a video the flush; with L >= the video's length
            emitted plus tail is the one-shot completed table;
  fill      what / glimpse / score of every emitted, tail and forecast row are bit copies of the source sighting's provider rows,
            which may lie in an earlier chunk: the provider's rows of the last D frames are carried.
The carried state (`new_smooth_state`; include/air_hip.h states the layout) is the smoother's own: frames_seen and the next frame to
emit per sequence; a table of at most 32 tracks derived from the chunk's track_id / num_objects / valid alone, which mirrors the
tracker's births and retirements with the same max_age (the tracker's state is only read); and rings over the last D global frames of
what the backward pass reads per (table row, frame) and of the provider's rows.  D = F + L + max_age (`ring_depth`): a push writes the
frames a .. a + F - 1 and emits from a - L on, and the source of a FILLED row there lies up to max_age frames before it; the reference
tags every ring entry with its frame and asserts the tag on every read.  The default lag (max_age) is provisional like the noise
terms.  Out of scope on a stream: smoothed covariances, motion-predicted association and its gate (track.py: MOTION, THE GATE; a stream
tracker would have to carry each slot's filter state), IDF1 and HOTA (their tables are indexed by global id).

NOISE FIT (`TrajectoryNoiseFitter` behind a track.SequenceTracker; air_track_noise_stats, air_track_noise_reduce; `reference_noise_stats`
restates both in numpy, bit for bit).  The forward filter above computes every innovation e = z - x- and its variance s = Pxx- + r: the
log-likelihood of a track's sightings after its first, given its first, is  l = -1/2 sum_updates sum_components [log 2 pi + log s +
e^2 / s]  (a track with one sighting and a coasted frame contribute nothing).  SCALE FAMILY: with the four terms written as
r (rho_shift, rho_scale, 1, nu), the rule at r = 1, q = rho, velocity_var = nu gives the same gains and innovations and s~ = s / r; with N
innovations, Q = sum e^2 / s~ and Lambda = sum log s~:  l(r) = -1/2 [N log(2 pi r) + Lambda + Q / r],  r^ = Q / N,
l^ = -1/2 [N (log(2 pi Q / N) + 1) + Lambda].  The covariances are per noise class, so Q = Q_0(rho_shift) + Q_1(rho_scale), Lambda alike,
and G evaluations per class give the G x G profile surface (`profile_fit`).  The device runs no transcendental function: per track and
class, at each update, s~ = Pxx- + 1, d = (e_a e_a + e_b e_b) / s~ (a < b the class's two components), Q = Q + d, and the product of
the s~ as a pair (m, k), value m 2^k, from (0.5, 1): (m_s, k_s) = frexp(s~), (m, j) = frexp(m m_s), k += k_s + j -- each s~ once, the
host doubles Lambda.  The combine order is fixed: a binary tree over the 64 lanes of a pass (strides 32 .. 1, lane i < stride takes lane
i + stride, idle lanes the identities 0.0 and (0.5, 1)), the passes, then the sequences, in ascending order, then the totals.  The
fit's domain is the smoother's (FIT_*), so a fitted setting is one `check_arguments` takes.  Out of scope: fitting on a stream;
fitting nu jointly (fit twice and compare `loglik`: comparable on the same tracks); noise terms per sequence; the association defaults.
"""
import ctypes
from collections import OrderedDict
from typing import Dict

from .stage import BoundStage, ReadOut, compacted_rows
from .track import MAX_GT, MAX_IDS, MAX_SLOTS, IdentityScores
from .track import check_arguments as check_track_arguments
from .track import check_frames_seen, check_valid

MAX_HORIZON = 16
MAX_LAG = 16                                                       # a stream smoother's lag L: max_age <= L <= MAX_LAG
ABSENT, OBSERVED, FILLED, FORECAST = range(4)
STATES = ("absent", "observed", "filled", "forecast")
DEFAULTS = dict(process_noise=(1e-4, 1e-4), measurement_noise=4e-4, velocity_var=0.04)
# THE SUPPORTED NOISE DOMAIN (csrc: TRAJ_Q_OVER_R_MIN .. TRAJ_R_MAX; DESIGN.md section 19 has the measurement).  The rule's float64
# chain forms covariance differences P- - k P- and a 2 x 2 inverse through det = Pxx- Pvv- - Pxv- Pxv-: it delivers the posterior mean
# to well under one float32 rounding of the output inside this box and loses digits, then turns NaN, outside it.  Outside: refused.
Q_OVER_R_MIN, Q_OVER_R_MAX = 1e-29, 1e15                           # process_noise / measurement_noise, each class
V_OVER_R_MAX = 1e6                                                 # velocity_var / measurement_noise (0 is inside)
R_MIN, R_MAX = 1e-146, 1e134                                       # measurement_noise


def completed_rows(max_steps, max_age) -> int:
    """C = min(32, T (max_age + 1)): a track that spans a frame without a sighting there was last seen in one of the max_age frames
    before it, and the live table holds at most 32 tracks"""
    return min(MAX_SLOTS, int(max_steps) * (int(max_age) + 1))


def check_arguments(max_steps, n_frames, n_rows=None, max_age=1, horizon=0, process_noise=DEFAULTS["process_noise"],
                    measurement_noise=DEFAULTS["measurement_noise"], velocity_var=DEFAULTS["velocity_var"], domain=True):
    """Refuse what air_track_smooth refuses (pure host code).  Returns (T, F, S, C, Hz, (q_shift, q_scale), r, velocity_var).
    domain=False keeps every check but the supported noise domain: `reference_smooth` and `reference_smooth_stream` pass it, because
    the restatement has to say what the rule's statements give for ANY positive noise -- the measurement of the domain, and the exact
    consequences that hold whatever the noise, run it where the device entries refuse.  Everything that launches uses domain=True."""
    T, F, S = check_track_arguments(max_steps, n_frames, n_rows, max_age=max_age)
    try:
        q = tuple(float(v) for v in process_noise)
    except TypeError:
        q = ()
    if len(q) != 2 or not all(v > 0.0 for v in q):
        raise ValueError("process_noise must be two positive numbers (q_shift, q_scale), got %r" % (process_noise,))
    r, vv = float(measurement_noise), float(velocity_var)
    if not r > 0.0:
        raise ValueError("measurement_noise must be a positive number, got %r" % (measurement_noise,))
    if not vv >= 0.0:
        raise ValueError("velocity_var must be a number >= 0, got %r" % (velocity_var,))
    if not domain:
        pass
    elif not R_MIN <= r <= R_MAX:
        raise ValueError("measurement_noise must lie within R_MIN..R_MAX = %g..%g, got %r" % (R_MIN, R_MAX, measurement_noise))
    elif not all(Q_OVER_R_MIN <= v / r <= Q_OVER_R_MAX for v in q):
        raise ValueError("process_noise / measurement_noise must lie within Q_OVER_R_MIN..Q_OVER_R_MAX = %g..%g (the float64 rule "
                         "loses the posterior mean outside), got %r / %r" % (Q_OVER_R_MIN, Q_OVER_R_MAX, process_noise, measurement_noise))
    elif not vv / r <= V_OVER_R_MAX:
        raise ValueError("velocity_var / measurement_noise must be at most V_OVER_R_MAX = %g (the float64 rule loses the posterior "
                         "mean beyond; an unknown velocity is velocity_var = V_OVER_R_MAX * measurement_noise), got %r / %r"
                         % (V_OVER_R_MAX, velocity_var, measurement_noise))
    if isinstance(horizon, bool) or int(horizon) != horizon or not 0 <= int(horizon) <= MAX_HORIZON:
        raise ValueError("horizon must be an integer within 0..%d, got %r" % (MAX_HORIZON, horizon))
    return T, F, S, completed_rows(T, max_age), int(horizon), q, r, vv


def _filter_start(z, r, vv):
    """start: the filtered state (x, v, Pxx, Pxv, Pvv) at the first sighting z (float64 [4], None: zeros)"""
    import numpy as np
    return (np.zeros(4) if z is None else z.copy(), np.zeros(4), np.full(4, r), np.zeros(4), np.full(4, vv))


def _filter_step(filt, z, q, r):
    """predict, then update with the sighting z (None: a coasted frame keeps the predicted state).  Returns (predicted, filtered)"""
    q2, q4 = 0.5 * q, 0.25 * q
    x, v, Pxx, Pxv, Pvv = filt
    a, b = Pxx + Pxv, Pxv + Pvv
    xp, vp = x + v, v
    Pxxp, Pxvp, Pvvp = (a + b) + q4, b + q2, Pvv + q
    pred = (xp, vp, Pxxp, Pxvp, Pvvp)
    if z is None:
        return pred, pred
    s = Pxxp + r
    kx, kv = Pxxp / s, Pxvp / s
    e = z - xp
    return pred, (xp + kx * e, vp + kv * e, Pxxp - kx * Pxxp, Pxvp - kx * Pxvp, Pvvp - kv * Pxvp)


def _back_step(filt, pred_next, xs_next, vs_next):
    """back: (xs, vs) of frame f from its filtered state, the predicted state of frame f + 1 and (xs, vs) of frame f + 1"""
    fx, fv, Pxx, Pxv, Pvv = filt
    xp, vp, Pxxp, Pxvp, Pvvp = pred_next
    g00, g01, g10, g11 = Pxx + Pxv, Pxv, Pxv + Pvv, Pvv
    det = Pxxp * Pvvp - Pxvp * Pxvp
    C00, C01 = (g00 * Pvvp - g01 * Pxvp) / det, (g01 * Pxxp - g00 * Pxvp) / det
    C10, C11 = (g10 * Pvvp - g11 * Pxvp) / det, (g11 * Pxxp - g10 * Pxvp) / det
    dx, dv = xs_next - xp, vs_next - vp
    return fx + (C00 * dx + C01 * dv), fv + (C10 * dx + C11 * dv)


def _smooth_track(z_of, first, last, q, r, vv):
    """the filter and the backward pass of one track: z_of(f) -> float64 [4] or None.  Returns xs, vs {f: [4]}, the filtered (x, v)
    at `last`, and the (frame, value) of every sighting"""
    filt, pred = {}, {}
    for f in range(first, last + 1):
        if f == first:
            filt[f] = _filter_start(z_of(f), r, vv)
        else:
            pred[f], filt[f] = _filter_step(filt[f - 1], z_of(f), q, r)
    x, v = filt[last][:2]
    xs, vs = {last: x}, {last: v}
    for f in range(last - 1, first - 1, -1):
        xs[f], vs[f] = _back_step(filt[f], pred[f + 1], xs[f + 1], vs[f + 1])
    return xs, vs, (x, v)


def _new_table(pre, C, cols):
    """an ABSENT table of C rows and `cols` columns under the prefix `pre`"""
    import numpy as np
    return {pre + "where": np.zeros((C, cols, 4), np.float32), pre + "boxes": np.zeros((C, cols, 4), np.float32),
            pre + "id": np.full((C, cols), -1, np.int32), pre + "state": np.zeros((C, cols), np.int8),
            pre + "src_frame": np.full((C, cols), -1, np.int32), pre + "src_slot": np.full((C, cols), -1, np.int32),
            pre + "velocity": np.zeros((C, cols, 2), np.float32), pre + "count": np.zeros(cols, np.int32)}


def _velocity(v, H, W):
    """pixels per frame of the box centre from the rates of tx and ty, float64 rounded once"""
    import numpy as np
    half = np.float64(0.5)
    return np.array([(np.float64(W) * v[1]) * half, (np.float64(H) * v[3]) * half]).astype(np.float32)


def _put(out, img_size, pre, row, col, w32, vel, tid, state, src):
    """one row of a table"""
    from .tile import scene_boxes
    out[pre + "where"][row, col], out[pre + "boxes"][row, col] = w32, scene_boxes(w32, img_size)
    out[pre + "velocity"][row, col], out[pre + "id"][row, col], out[pre + "state"][row, col] = vel, tid, state
    out[pre + "src_frame"][row, col], out[pre + "src_slot"][row, col] = src
    out[pre + "count"][col] = max(out[pre + "count"][col], row + 1)


def _forecast_where(xl, vl, m):
    """the forecast m frames past the last sighting: shifts extrapolated from the filtered (x, v) at `last`, scales held"""
    import numpy as np
    m = np.float64(m)
    return np.array([xl[0], xl[1] + m * vl[1], xl[2], xl[3] + m * vl[3]]).astype(np.float32)


def reference_smooth(where, num_objects, track_id, num_tracks, track_first, track_last, n_frames, max_age, img_size, horizon=0,
                     process_noise=DEFAULTS["process_noise"], measurement_noise=DEFAULTS["measurement_noise"],
                     velocity_var=DEFAULTS["velocity_var"], what=None, glimpse=None, score=None):
    """air_track_smooth (and, with what [T, R, A], glimpse [T, R, G] and score [T, R] given, air_track_fill) restated in numpy float64.
    where [T, R, 4] fp32, num_objects [R], track_id [T, R], num_tracks [S], track_first / track_last [S, F T], R = S n_frames.
    Returns sm_where, sm_boxes [C, R, 4] float32, sm_id [C, R] int32, sm_state [C, R] int8, sm_src_frame, sm_src_slot [C, R] int32,
    sm_velocity [C, R, 2] float32, sm_count [R], sm_counts [S, 3] int32, the same with fc_ and [C, S Hz] for the forecast table
    (fc_count [S Hz]), and sm_what / sm_glimpse / sm_score / fc_what / fc_glimpse / fc_score when the rows to copy are given.
    Tables no tracker writes (the entry takes any integers; include/air_hip.h pins the same): num_tracks is clipped to 0 .. F T, a track
    with first < 0, first > last or last >= F is skipped, a table row no slot names is a track without sightings (FILLED from z = 0),
    of two slots that carry one id the lowest is read, and a row counts the ids below whose `last` reaches the frame whatever their
    `first`.  The device keeps the 32 lowest such ids per track, as a tracker's live table does: with a 33rd, the rows are the
    device's only in the frames the ids beyond the 32 lowest do not reach."""
    import numpy as np
    from .tile import scene_boxes
    where = np.asarray(where, np.float32)
    T, R = where.shape[:2]
    T, F, S, C, Hz, (q_shift, q_scale), r, vv = check_arguments(T, n_frames, R, max_age, horizon, process_noise, measurement_noise,
                                                                velocity_var, domain=False)
    H, W = (int(v) for v in img_size)
    ids, n_in = np.asarray(track_id).astype(np.int64), np.asarray(num_objects).astype(np.int64)
    FT, N = F * T, S * Hz
    first, last = np.asarray(track_first).reshape(S, FT).astype(np.int64), np.asarray(track_last).reshape(S, FT).astype(np.int64)
    q = np.array([q_scale, q_shift, q_scale, q_shift], np.float64)
    out = {}
    for pre, cols in (("sm_", R), ("fc_", N)):
        out.update(_new_table(pre, C, cols))
    out["sm_counts"] = np.zeros((S, 3), np.int32)
    velocity = lambda v: _velocity(v, H, W)
    put = lambda *a: _put(out, (H, W), *a)

    with np.errstate(all="ignore"):
        for s in range(S):
            issued = int(min(max(int(np.asarray(num_tracks)[s]), 0), FT))
            valid = [i for i in range(issued) if 0 <= first[s, i] <= last[s, i] < F]

            def sighting(i, f):
                rr = s * F + f
                n = int(min(max(n_in[rr], 0), T))
                return next((j for j in range(n) if ids[j, rr] == i), None)

            for i in valid:
                fi, la = int(first[s, i]), int(last[s, i])
                slots = {f: sighting(i, f) for f in range(fi, la + 1)}
                z_of = lambda f: None if slots[f] is None else where[slots[f], s * F + f].astype(np.float64)
                xs, vs, (xl, vl) = _smooth_track(z_of, fi, la, q, r, vv)
                src = (-1, -1)
                for f in range(fi, la + 1):
                    if slots[f] is not None:
                        src = (f, slots[f])
                    row = sum(1 for k in valid if k < i and last[s, k] >= f)
                    if row >= C:
                        continue
                    state = OBSERVED if slots[f] is not None else FILLED
                    put("sm_", row, s * F + f, xs[f].astype(np.float32), velocity(vs[f]), i, state, src)
                    out["sm_counts"][s, state] += 1
                if Hz > 0 and F - 1 - la <= max_age:
                    row = sum(1 for k in valid if k < i and F - 1 - last[s, k] <= max_age)
                    if row >= C:
                        continue
                    for k in range(1, Hz + 1):
                        put("fc_", row, s * Hz + (k - 1), _forecast_where(xl, vl, F - 1 - la + k), velocity(vl), i, FORECAST, src)
            out["sm_counts"][s, ABSENT] = C * F - out["sm_counts"][s, OBSERVED] - out["sm_counts"][s, FILLED]
    if what is not None:
        rows = {"what": np.asarray(what, np.float32), "glimpse": np.asarray(glimpse, np.float32).reshape(T, R, -1),
                "score": np.asarray(score, np.float32)}
        for pre, cols, per_seq in (("sm_", R, F), ("fc_", N, Hz)):
            for k, src_rows in rows.items():
                dst = np.zeros((C, cols) + src_rows.shape[2:], np.float32)
                for c in range(C):
                    for n in range(cols):
                        sf, sj = out[pre + "src_frame"][c, n], out[pre + "src_slot"][c, n]
                        if out[pre + "state"][c, n] != ABSENT and 0 <= sf < F and 0 <= sj < T:
                            dst[c, n] = src_rows[sj, (n // per_seq) * F + sf]
                out[pre + k] = dst
    return out


# ---- streams: fixed-lag smoothing and forecasts per chunk (the module text and include/air_hip.h state the rule and the layout) --------
SM_LIVE, SM_ID, SM_AGE, SM_FIRST, SM_LAST_FRAME, SM_LAST_SLOT = range(6)
SM_FIELDS = ("live", "id", "age", "first", "last_frame", "last_slot")
SM_EMPTY = (0, -1, 0, -1, -1, -1)                                  # a table row that is not live, field by field
RING_ID, RING_STATE, RING_SRC_FRAME, RING_SRC_SLOT = range(4)
RING_EMPTY = (-1, ABSENT, -1, -1)                                  # a table row that was not live in that frame
WS_DOUBLES = 28                                                    # TRAJ_WS_DOUBLES: 4 x (x, v, x-, v-), 2 noise classes x (P, P-)
SMOOTH_STATE_KEYS = ("seq", "slots", "ring_i", "ring")             # the packed device state, in this order
ROW_RING_KEYS = ("what", "glimpse", "score")                       # the ring of provider rows (three buffers of their own)
_CLASS = (1, 0, 1, 0)                                              # [sx, tx, sy, ty]: noise class 0 the shifts, 1 the scales


def ring_depth(chunk_frames, lag, max_age) -> int:
    """D = F + L + max_age frames.  A push that starts at frames_seen = a writes the frames a .. a + F - 1 and emits from a - L on;
    the FILLED row of a track that coasts there has its source sighting up to max_age frames earlier: a - L - max_age is the oldest
    frame read, a + F - 1 the newest written"""
    return int(chunk_frames) + int(lag) + int(max_age)


def check_stream_arguments(max_steps, chunk_frames, n_rows=None, max_age=1, lag=None, horizon=0,
                           process_noise=DEFAULTS["process_noise"], measurement_noise=DEFAULTS["measurement_noise"],
                           velocity_var=DEFAULTS["velocity_var"], domain=True):
    """Refuse what air_track_smooth_stream refuses (pure host code).  lag=None: max_age.  Returns (T, F, S, C, L, Hz, D, (q_shift,
    q_scale), r, velocity_var).  domain: as `check_arguments`."""
    T, F, S, C, Hz, q, r, vv = check_arguments(max_steps, chunk_frames, n_rows, max_age, horizon, process_noise, measurement_noise,
                                               velocity_var, domain)
    lag = int(max_age) if lag is None else lag
    if isinstance(lag, bool) or int(lag) != lag or not int(max_age) <= int(lag) <= MAX_LAG:
        raise ValueError("lag must be an integer within max_age..%d = %d..%d (a track that coasts over a frame must be retired, or "
                         "seen again, by the time the frame is emitted), got %r" % (MAX_LAG, int(max_age), MAX_LAG, lag))
    return T, F, S, C, int(lag), Hz, ring_depth(F, lag, max_age), q, r, vv


def new_smooth_state(n_sequences, chunk_frames, lag, max_age, max_steps, what_size, glimpse_size, depth=None):
    """the smoother state of a stream that has seen nothing, as numpy arrays.  The packed device state (SMOOTH_STATE_KEYS): seq [S, 2]
    int32 {frames_seen, next frame to emit}, slots [S, 6, 32] int32 (SM_FIELDS), ring_i [S, D, 4, 32] int32 {id, state, src_frame,
    src_slot} and ring [S, D, 28, 32] float64 over the frames g at g mod D.  The ring of provider rows (ROW_RING_KEYS): what
    [S, D, T, A], glimpse [S, D, T, G], score [S, D, T] fp32.  Host bookkeeping only: ring_frame, rows_frame [S, D] int64, the frame a
    ring entry holds (-1: none), which the reference asserts on every read.  depth: D, `ring_depth` if None."""
    import numpy as np
    S, T, A, G = int(n_sequences), int(max_steps), int(what_size), int(glimpse_size)
    D = ring_depth(chunk_frames, lag, max_age) if depth is None else int(depth)
    slots, ring_i = np.empty((S, 6, MAX_SLOTS), np.int32), np.empty((S, D, 4, MAX_SLOTS), np.int32)
    slots[:] = np.asarray(SM_EMPTY, np.int32)[None, :, None]
    ring_i[:] = np.asarray(RING_EMPTY, np.int32)[None, None, :, None]
    return {"seq": np.zeros((S, 2), np.int32), "slots": slots, "ring_i": ring_i, "ring": np.zeros((S, D, WS_DOUBLES, MAX_SLOTS)),
            "what": np.zeros((S, D, T, A), np.float32), "glimpse": np.zeros((S, D, T, G), np.float32),
            "score": np.zeros((S, D, T), np.float32), "ring_frame": np.full((S, D), -1, np.int64),
            "rows_frame": np.full((S, D), -1, np.int64)}


def reset_smooth_state(state, sequences=None):
    """restart all (None) or some sequences of a numpy smoother state, in place"""
    import numpy as np
    S, D = state["ring"].shape[:2]
    rows = np.arange(S) if sequences is None else np.atleast_1d(np.asarray(sequences, np.int64))
    if rows.size and (rows.min() < 0 or rows.max() >= S):
        raise ValueError("reset: sequences within 0..%d, got %r" % (S - 1, sequences))
    fresh = new_smooth_state(1, 0, 0, 0, state["score"].shape[2], state["what"].shape[3], state["glimpse"].shape[3], depth=D)
    for k, v in fresh.items():
        state[k][rows] = v[0]
    return state


def smooth_state_layout(n_sequences, depth):
    """{key: (byte offset, dtype, shape)} of the packed device state and its size in bytes (air_track_smooth_stream_state_bytes)"""
    import numpy as np
    S, D = int(n_sequences), int(depth)
    shapes = (("seq", np.int32, (S, 2)), ("slots", np.int32, (S, 6, MAX_SLOTS)), ("ring_i", np.int32, (S, D, 4, MAX_SLOTS)),
              ("ring", np.float64, (S, D, WS_DOUBLES, MAX_SLOTS)))
    at, layout = 0, {}
    for k, dtype, shape in shapes:
        layout[k] = (at, dtype, shape)
        at += int(np.prod(shape)) * np.dtype(dtype).itemsize
    return layout, at


def pack_smooth_state(state):
    """the packed device state of a numpy state: uint8 [state bytes]"""
    import numpy as np
    return np.concatenate([np.ascontiguousarray(state[k]).reshape(-1).view(np.uint8) for k in SMOOTH_STATE_KEYS])


def unpack_smooth_state(packed, n_sequences, depth):
    """{key: array} (copies) of a packed device state"""
    import numpy as np
    layout, size = smooth_state_layout(n_sequences, depth)
    packed = np.ascontiguousarray(packed).reshape(-1).view(np.uint8)
    if packed.size != size:
        raise ValueError("a packed smoother state of %d sequences at depth %d has %d bytes, got %d" % (n_sequences, depth, size, packed.size))
    return {k: packed[at:at + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape).copy()
            for k, (at, dtype, shape) in layout.items()}


def _ring_put(plane, k, filt, pred):
    """the filtered and predicted state of table row k into one frame's planes [28, 32] (csrc: WS_X, WS_V, WS_XP, WS_VP, WS_P, WS_PP)"""
    plane[0:4, k], plane[4:8, k], plane[8:12, k], plane[12:16, k] = filt[0], filt[1], pred[0], pred[1]
    for c, comp in ((0, 1), (1, 0)):                               # class 0 from tx, class 1 from sx: ty and sy hold the same bits
        for i in range(3):
            plane[16 + 6 * c + i, k], plane[19 + 6 * c + i, k] = filt[2 + i][comp], pred[2 + i][comp]


def _ring_get(plane, k):
    import numpy as np
    cov = lambda base: tuple(np.array([plane[base + 6 * _CLASS[c] + i, k] for c in range(4)]) for i in range(3))
    return (plane[0:4, k].copy(), plane[4:8, k].copy()) + cov(16), (plane[8:12, k].copy(), plane[12:16, k].copy()) + cov(19)


def _ring_at(state, s, g, rows=False):
    """the ring index of global frame g, the host's tag asserted: a ring too shallow has overwritten the frame"""
    D = state["ring"].shape[1]
    tag = state["rows_frame" if rows else "ring_frame"][s, g % D]
    assert tag == g, "the ring of depth %d holds frame %d where frame %d is read: too shallow" % (D, tag, g)
    return g % D


def _stream_rows(state, s, g, hi):
    """the rows of frame g given the frames up to hi: [(id, table row, last sighting within g .. hi, state, src_frame, src_slot)] in
    ascending id of the tracks live in g that are sighted in g .. hi"""
    ri = state["ring_i"][s]
    found = []
    for k in range(MAX_SLOTS):
        tid, st, sf, sj = (int(v) for v in ri[_ring_at(state, s, g), :, k])
        if tid < 0:
            continue
        la = None
        for f in range(g, hi + 1):
            e = ri[_ring_at(state, s, f), :, k]
            if e[RING_ID] != tid:
                break
            if e[RING_STATE] == OBSERVED:
                la = f
        if la is not None:
            found.append((tid, k, la, st, sf, sj))
    return sorted(found)


def _stream_column(state, out, pre, s, col, g, hi, C, img_size):
    """frame g smoothed with the frames up to hi into column `col` of table `pre`: the backward pass from the track's last sighting
    within g .. hi down to g over the ring.  Returns the rows written per state"""
    H, W = img_size
    counts = [0, 0, 0]
    for row, (tid, k, la, st, sf, sj) in enumerate(_stream_rows(state, s, g, hi)):
        if row >= C:
            continue
        filt, _ = _ring_get(state["ring"][s, _ring_at(state, s, la)], k)
        xs, vs = filt[0], filt[1]
        for f in range(la - 1, g - 1, -1):
            filt, _ = _ring_get(state["ring"][s, _ring_at(state, s, f)], k)
            _, pred = _ring_get(state["ring"][s, _ring_at(state, s, f + 1)], k)
            xs, vs = _back_step(filt, pred, xs, vs)
        _put(out, (H, W), pre, row, col, xs.astype("float32"), _velocity(vs, H, W), tid, st, (sf, sj))
        counts[st] += 1
    return counts


def _stream_fill(state, out, pre, cols, per_seq, T):
    """what / glimpse / score of a table's rows from the ring of provider rows: bit copies of the source sighting's rows"""
    import numpy as np
    C = out[pre + "id"].shape[0]
    for key in ROW_RING_KEYS:
        out[pre + key] = np.zeros((C, cols) + state[key].shape[3:], np.float32)
    for c in range(C):
        for n in range(cols):
            sf, sj = int(out[pre + "src_frame"][c, n]), int(out[pre + "src_slot"][c, n])
            if out[pre + "state"][c, n] != ABSENT and sf >= 0 and 0 <= sj < T:
                s = n // per_seq
                for key in ROW_RING_KEYS:
                    out[pre + key][c, n] = state[key][s, _ring_at(state, s, sf, rows=True), sj]


def reference_smooth_stream(state, where, num_objects, track_id, n_frames, valid=None, lag=None, max_age=1, img_size=(50, 50), horizon=0,
                            process_noise=DEFAULTS["process_noise"], measurement_noise=DEFAULTS["measurement_noise"],
                            velocity_var=DEFAULTS["velocity_var"], what=None, glimpse=None, score=None):
    """air_track_stash, air_track_smooth_stream and air_track_fill_stream restated in numpy float64, on `_smooth_track`'s steps and
    `reference_smooth`'s table code: ONE chunk.  state: None (a stream starts) or what an earlier call returned (it is not modified);
    where [T, R, 4], num_objects [R], track_id [T, R] as the stream tracker leaves them, R = S n_frames, valid [S] (None: every frame);
    what [T, R, A], glimpse [T, R, G], score [T, R] (None: the row ring is left alone and no row is filled).  Returns (outputs, state):
    the emitted table sm_where .. sm_count at [C, S F] columns s F + e, e the order of emission, emit_frame [S, F] (GLOBAL, -1: none),
    num_emitted [S], sm_counts [S, 3] (over the emitted columns), the forecast table fc_ at [C, S Hz], with the rows given sm_what /
    sm_glimpse / sm_score and fc_ alike; and the new state (new_smooth_state's arrays)."""
    import numpy as np
    where = np.asarray(where, np.float32)
    T, R = where.shape[:2]
    T, F, S, C, L, Hz, D, (q_shift, q_scale), r, vv = check_stream_arguments(T, n_frames, R, max_age, lag, horizon, process_noise,
                                                                             measurement_noise, velocity_var, domain=False)
    H, W = (int(v) for v in img_size)
    ids, n_in = np.asarray(track_id).astype(np.int64), np.asarray(num_objects).astype(np.int64)
    v_in = check_valid(valid, S, F)
    rows = None if what is None else {"what": np.asarray(what, np.float32), "glimpse": np.asarray(glimpse, np.float32).reshape(T, R, -1),
                                      "score": np.asarray(score, np.float32)}
    if state is None:
        A, G = (rows["what"].shape[2], rows["glimpse"].shape[2]) if rows else (1, 1)
        state = new_smooth_state(S, F, L, max_age, T, A, G)
    else:
        state = {k: np.array(v) for k, v in state.items()}
    D = state["ring"].shape[1] if state["ring"].ndim == 4 else -1
    want = new_smooth_state(S, 1, 0, 0, T, state["what"].shape[-1], state["glimpse"].shape[-1], depth=max(D, 1))
    for k, v in want.items():
        if state[k].shape != v.shape or state[k].dtype != v.dtype:
            raise ValueError("the state's %s is %s %s; a chunk of %d sequences and %d rows per frame needs %s %s"
                             % (k, state[k].shape, state[k].dtype, S, T, v.shape, v.dtype))
    if rows and (rows["what"].shape[2] != state["what"].shape[3] or rows["glimpse"].shape[2] != state["glimpse"].shape[3]):
        raise ValueError("the state carries what rows of %d and glimpses of %d values, the chunk has %d and %d"
                         % (state["what"].shape[3], state["glimpse"].shape[3], rows["what"].shape[2], rows["glimpse"].shape[2]))
    check_frames_seen(state["seq"][:, 0], v_in)
    q = np.array([q_scale, q_shift, q_scale, q_shift], np.float64)
    N = S * Hz
    out = dict(_new_table("sm_", C, R), **_new_table("fc_", C, N))
    out.update(sm_counts=np.zeros((S, 3), np.int32), emit_frame=np.full((S, F), -1, np.int32), num_emitted=np.zeros(S, np.int32))
    zeros5 = tuple(np.zeros(4) for _ in range(5))
    with np.errstate(all="ignore"):
        for s in range(S):
            a, v = int(state["seq"][s, 0]), int(v_in[s])
            b = a + v
            sl, ring, ring_i = state["slots"][s], state["ring"][s], state["ring_i"][s]
            for f in range(v):                                     # ---- forward: the table and the rings, frame by frame
                g, rr = a + f, s * F + f
                d = g % D
                if rows:
                    for key in ROW_RING_KEYS:
                        state[key][s, d] = rows[key][:, rr]
                    state["rows_frame"][s, d] = g
                n = int(min(max(n_in[rr], 0), T))
                seen, born = {}, set()
                for j in range(n):                                 # sightings by id in ascending slot; births into the lowest free row
                    i = int(ids[j, rr])
                    if i < 0:
                        continue
                    k = next((k for k in range(MAX_SLOTS) if sl[SM_LIVE, k] and sl[SM_ID, k] == i), None)
                    if k is None:
                        k = next((k for k in range(MAX_SLOTS) if not sl[SM_LIVE, k]), None)
                        if k is None:
                            continue                               # (33 live ids: no tracker writes them)
                        sl[:, k] = (1, i, 0, g, -1, -1)
                        born.add(k)
                        seen[k] = j
                    elif k not in seen:
                        seen[k] = j
                for k in range(MAX_SLOTS):
                    if not sl[SM_LIVE, k]:
                        ring_i[d, :, k] = RING_EMPTY
                        continue
                    z = where[seen[k], rr].astype(np.float64) if k in seen else None
                    if k in born:
                        pred, filt = zeros5, _filter_start(z, r, vv)
                    else:
                        pred, filt = _filter_step(_ring_get(ring[_ring_at(state, s, g - 1)], k)[0], z, q, r)
                    if k in seen:
                        sl[SM_AGE, k], sl[SM_LAST_FRAME, k], sl[SM_LAST_SLOT, k] = 0, g, seen[k]
                    else:
                        sl[SM_AGE, k] += 1
                    _ring_put(ring[d], k, filt, pred)
                    ring_i[d, :, k] = (sl[SM_ID, k], OBSERVED if k in seen else FILLED, sl[SM_LAST_FRAME, k], sl[SM_LAST_SLOT, k])
                state["ring_frame"][s, d] = g
                for k in range(MAX_SLOTS):                         # retirement: the tracker's ageing
                    if sl[SM_LIVE, k] and sl[SM_AGE, k] > max_age:
                        sl[:, k] = SM_EMPTY
            e = 0                                                  # ---- the frames that became final: g + L < b
            for g in range(int(state["seq"][s, 1]), max(0, b - L)):
                counts = _stream_column(state, out, "sm_", s, s * F + e, g, g + L, C, (H, W))
                out["sm_counts"][s, OBSERVED] += counts[OBSERVED]
                out["sm_counts"][s, FILLED] += counts[FILLED]
                out["emit_frame"][s, e] = g
                e += 1
            assert e <= F
            out["num_emitted"][s] = e
            out["sm_counts"][s, ABSENT] = C * e - out["sm_counts"][s, OBSERVED] - out["sm_counts"][s, FILLED]
            state["seq"][s] = (b, max(0, b - L))
            live = sorted((int(sl[SM_ID, k]), k) for k in range(MAX_SLOTS) if sl[SM_LIVE, k])      # ---- the forecast
            for row, (tid, k) in enumerate(live if Hz and b else []):
                if row >= C:
                    continue
                la = int(sl[SM_LAST_FRAME, k])
                (xl, vl) = _ring_get(ring[_ring_at(state, s, la)], k)[0][:2]
                for kk in range(1, Hz + 1):
                    _put(out, (H, W), "fc_", row, s * Hz + (kk - 1), _forecast_where(xl, vl, b - 1 - la + kk), _velocity(vl, H, W), tid,
                         FORECAST, (la, int(sl[SM_LAST_SLOT, k])))
        if rows:
            _stream_fill(state, out, "sm_", R, F, T)
            _stream_fill(state, out, "fc_", N, max(Hz, 1), T)
    return out, state


def reference_smooth_tail(state, lag, max_age, img_size, fill=True):
    """air_track_smooth_tail (and, fill=True, air_track_fill_stream on it) restated: the frames max(0, b - L) .. b - 1 of every
    sequence, not final yet, smoothed with what is known -- the last columns of `reference_smooth` on the first b frames.  The state
    is only read.  Returns tl_where .. tl_count at [C, S L] columns s L + j, tail_frame [S, L] (GLOBAL, -1: none), num_tail [S]."""
    import numpy as np
    S, D, T = state["score"].shape
    L, C = int(lag), completed_rows(T, max_age)
    cols = S * L
    out = _new_table("tl_", C, cols)
    out.update(tail_frame=np.full((S, L), -1, np.int32), num_tail=np.zeros(S, np.int32))
    with np.errstate(all="ignore"):
        for s in range(S):
            b = int(state["seq"][s, 0])
            for j, g in enumerate(range(max(0, b - L), b)):
                _stream_column(state, out, "tl_", s, s * L + j, g, b - 1, C, tuple(int(v) for v in img_size))
                out["tail_frame"][s, j] = g
                out["num_tail"][s] = j + 1
        if fill:
            _stream_fill(state, out, "tl_", cols, max(L, 1), T)
    return out


class CompletedFrames:
    """The completed frames of a TrajectorySmoother as a provider: what [C, R, A], where [C, R, 4], glimpse [C, R, G], boxes [C, R, 4],
    score, presence [C, R], num_objects [R], owner [R, H, W], T = C, R, engine, mask_threshold -- what score.ParseScorer reads, so it
    binds to this unchanged.  (The smoother itself carries the same buffers, but its `score` is the identity metric's method.)"""
    KIND = "completed"

    def __init__(self, smoother):
        t = smoother.sm
        self.smoother, self.engine, self.T, self.R = smoother, smoother.engine, smoother.C, smoother.R
        self.what, self.where, self.glimpse, self.boxes, self.score = t["what"], t["where"], t["glimpse"], t["boxes_out"], t["score_out"]
        self.presence, self.num_objects, self.owner = t["presence"], t["num_objects"], t["owner"]
        self.mask_threshold = smoother.mask_threshold

    def rows(self):
        """the provider protocol (stage.py): the completed rows; there is no count posterior and no image of a completed frame"""
        return compacted_rows(self, None, None)

    def launch_count(self):
        return self.smoother.launch_count()

    def synchronize(self):
        self.engine.synchronize()


def _table_result(pre, t, C, crop_size):
    """the tensors of one table (TrajectorySmoother._table) under the prefix `pre`, the glimpses viewed as crops"""
    out = {pre + k: t[k] for k in ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity", "count", "what", "score",
                                   "presence", "offsets", "obj_image", "obj_step", "obj_box", "obj_score", "obj_where", "obj_what",
                                   "reconstruction", "owner", "area")}
    out[pre + "glimpse"] = t["glimpse"].view(C, t["count"].shape[0], *crop_size)
    return out


class TrajectorySmoother(BoundStage):
    """binds to a SequenceTracker (what it forwards parameters and switches to) and reads that tracker's provider"""
    KEY_FIELDS = ("output_multiplier", "output_std")

    def __init__(self, tracker, horizon=0, process_noise=DEFAULTS["process_noise"], measurement_noise=DEFAULTS["measurement_noise"],
                 velocity_var=DEFAULTS["velocity_var"]):
        provider = tracker.provider
        T, F, S, C, Hz, q, r, vv = check_arguments(tracker.T, tracker.F, tracker.R, tracker.max_age, horizon, process_noise,
                                                   measurement_noise, velocity_var)
        import torch
        from . import hip as H
        self.tracker, self.provider, self.engine = tracker, provider, tracker.engine
        self.parser = provider
        self._bound = tracker
        self.window_T, self.T, self.C, self.R, self.S, self.F, self.horizon = T, C, C, int(tracker.R), S, F, Hz
        self.process_noise, self.measurement_noise, self.velocity_var, self.max_age = q, r, vv, int(tracker.max_age)
        self.mask_threshold = provider.mask_threshold
        self.img_size = tuple(tracker.img_size)
        self._rows = {k: tracker._rows[k] for k in ("what", "where", "glimpse")}
        cfg = self.engine.cfg
        self.A, self.G = int(tracker.A), int(cfg.crop_size[0]) * int(cfg.crop_size[1])
        dev, R, N = self.engine.device, self.R, S * Hz
        L = H.lib()
        self.n_bands = int(L.air_canvas_unroll_bands(R, self.img_size[0]))
        self.n_bands_fc = int(L.air_canvas_unroll_bands(N, self.img_size[0])) if N else 0
        self.workspace_bytes = int(L.air_track_smooth_workspace_bytes(C, R))
        self._H = H
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.workspace = z((self.workspace_bytes // 8,), torch.float64)
            (self.sm, self._sm_ro), (self.fc, self._fc_ro) = self._table(z, R, self.n_bands), \
                (self._table(z, N, self.n_bands_fc) if N else (None, None))
            self.sm_counts = z((S, 3), torch.int32)
        self.scores = IdentityScores(self, S)
        self._score = self.scores.entries                          # (table, G, tau) -> buffers, plan, graph
        self.totals_i, self.totals_f = self.scores.totals_i, self.scores.totals_f
        # the provider surface: the completed frames (`score` is this object's scoring method: the per-row score tensor is
        # `completed.score`, and `completed` is what a score.ParseScorer binds to)
        t = self.sm
        self.what, self.where, self.glimpse, self.boxes = t["what"], t["where"], t["glimpse"], t["boxes_out"]
        self.presence, self.num_objects, self.owner = t["presence"], t["num_objects"], t["owner"]
        self.completed = CompletedFrames(self)
        self._rebuild()
        for name in ("readout", "readout_forecast"):               # (tile.py's rule)
            if name in self.segments:
                self.check_render(self.segments[name][2],
                                  "air_parse_render declines %d x %d frames with %d completed rows: its LDS carve passes the 160 KiB "
                                  "of a workgroup; use a smaller max_age" % (self.img_size + (self.C,)))
        self.engine.synchronize()

    def _table(self, z, N, n_bands):
        """the buffers of one table of C rows and N columns: air_track_smooth's and air_track_fill's outputs, and the read-out (what
        the parsers keep; its score and boxes under score_out / boxes_out)"""
        import torch
        C, A, G = self.C, self.A, self.G
        ro = ReadOut(self._H, self.engine, C, N, A, self.img_size, n_bands, self.mask_threshold, with_rec=False)
        t = {"where": z((C, N, 4)), "boxes": z((C, N, 4)), "id": z((C, N), torch.int32), "state": z((C, N), torch.int8),
             "src_frame": z((C, N), torch.int32), "src_slot": z((C, N), torch.int32), "velocity": z((C, N, 2)),
             "count": z((N,), torch.int32), "what": z((C, N, A)), "glimpse": z((C, N, G)), "score": z((C, N))}
        t.update(ro.tensors(score="score_out", boxes="boxes_out"))
        return t, ro

    # ---- the launches behind the tracker's own -------------------------------------------------------------------------------
    def _readout(self, t, ro):
        return [ro.objects(None, t["count"], t["where"], t["what"]), ro.relabel("air_tile_relabel", t["score"], t["id"]),
                ro.render(t["glimpse"], t["where"], None)]

    def _fill(self, t, N, per_seq):
        H, rows, par = self._H, self._rows, self.provider
        L, p = H.lib(), H._p
        return [(L.air_track_fill,
                 (p(rows["what"]), p(rows["glimpse"]), p(par.score), p(t["state"]), p(t["src_frame"]), p(t["src_slot"]), self.window_T,
                  self.F, self.R, self.C, N, per_seq, self.A, self.G, p(t["what"]), p(t["glimpse"]), p(t["score"])), "air_track_fill")]

    def _build_plan(self):
        H, tk, par, rows = self._H, self.tracker, self.provider, self._rows
        L, p, size = H.lib(), H._p, ctypes.c_size_t
        Hi, Wi = self.img_size
        sm, fc, Hz = self.sm, self.fc, self.horizon
        fcp = lambda k: p(fc[k]) if fc is not None else None
        qs, qc = self.process_noise
        self.segments = OrderedDict([
            ("smooth", [(L.air_track_smooth,
                         (p(rows["where"]), p(par.num_objects), p(tk.track_id), p(tk.num_tracks), p(tk.track_first), p(tk.track_last),
                          self.window_T, self.S, self.F, self.R, self.C, Hz, self.max_age, Hi, Wi, qs, qc, self.measurement_noise,
                          self.velocity_var, p(self.workspace), size(self.workspace_bytes), p(sm["where"]), p(sm["boxes"]), p(sm["id"]),
                          p(sm["state"]), p(sm["src_frame"]), p(sm["src_slot"]), p(sm["velocity"]), p(sm["count"]), p(self.sm_counts),
                          fcp("where"), fcp("boxes"), fcp("id"), fcp("state"), fcp("src_frame"), fcp("src_slot"), fcp("velocity"),
                          fcp("count")), "air_track_smooth")]),
            ("fill", self._fill(sm, self.R, self.F)),
            ("readout", self._readout(sm, self._sm_ro))])
        if fc is not None:
            self.segments["fill_forecast"] = self._fill(fc, self.S * Hz, Hz)
            self.segments["readout_forecast"] = self._readout(fc, self._fc_ro)
        self._plan = [e for seg in self.segments.values() for e in seg]

    def _score_entries(self):
        return self.scores.score_entries()

    def launch_count(self) -> Dict[str, int]:
        """entries of one `run()` behind the tracker's own (`tracker` holds that tracker's launch_count())"""
        n = 2 if self.fc is not None else 1
        return {"tracker": self.tracker.launch_count(), "track_smooth": 1, "track_fill": n, "parse_objects": n, "tile_relabel": n,
                "parse_render": n}

    # ---- the trajectories ---------------------------------------------------------------------------------------------------
    def run(self, base=None):
        """the trajectories of the tracker's LATEST `track()`; `base` (that call's result) is passed through into the returned dict.
        The tracker's and the provider's buffers are only read.  Same stream contract as SequenceTracker.track."""
        eng = self.engine
        self._refresh_plan()
        eng.wait_for_caller()
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        return self.result(base)

    def track(self, frames, *args, **kwargs):
        """the bound tracker's `track(frames, ...)`, then `run()` on its result"""
        return self.run(self.tracker.track(frames, *args, **kwargs))

    def result(self, base=None):
        """Device tensors that the NEXT call overwrites, next to `base`.  The completed table, C rows per frame: sm_where, sm_boxes
        [C, R, 4], sm_id [C, R] int32 (-1 = none), sm_state [C, R] int8 (STATES), sm_src_frame, sm_src_slot [C, R] int32, sm_velocity
        [C, R, 2] (pixels per frame of the box centre), sm_count [R], sm_counts [S, 3] int32, sm_what [C, R, A], sm_glimpse
        [C, R, h, w], sm_score [C, R] (the source sighting's), and its read-out: sm_presence [C, R], sm_offsets, sm_obj_image,
        sm_obj_step (the track id), sm_obj_box, sm_obj_score, sm_obj_where, sm_obj_what, sm_reconstruction [R, H, W], sm_owner
        [R, H, W] int8 (the ROW that owns a pixel), sm_area [C, R].  With a horizon: the same under fc_ at [C, S Hz] columns
        s Hz + (k - 1), and frames_pred [S, Hz, H, W]."""
        cfg = self.engine.cfg
        out = dict(base) if base is not None else {}
        for pre, t in (("sm_", self.sm), ("fc_", self.fc)):
            if t is not None:
                out.update(_table_result(pre, t, self.C, cfg.crop_size))
        out["sm_counts"] = self.sm_counts
        if self.fc is not None:
            out["frames_pred"] = self.fc["reconstruction"].view(self.S, self.horizon, *self.img_size)
        return out

    # ---- the identity metric on the tables ------------------------------------------------------------------------------------
    def _score_table(self, table, entry):
        """the completed or the forecast table as IdentityScores takes one; `entry` names the kernel in the refusal"""
        t, n_frames = (self.sm, self.F) if table == "completed" else (self.fc, self.horizon)
        if n_frames * self.C > MAX_IDS:
            raise ValueError("%s takes at most %d rows per sequence; %d frames of %d completed rows are %d"
                             % (entry, MAX_IDS, n_frames, self.C, n_frames * self.C))
        return (self.C, n_frames, t["boxes"], t["count"], t["id"])

    def _score_entry(self, table, G, tau, identity=False):
        return self.scores.entry((table,), G, tau, self._score_table(table, "air_track_score"), identity, self.F * self.window_T)

    def _run_score(self, table, gt_boxes, tau, n_frames, identity=False):
        return self.scores.run(gt_boxes, n_frames, lambda G: self._score_entry(table, G, tau, bool(identity)))

    def score(self, gt_boxes, tau=0.5, accumulate=True, identity=False):
        """SequenceTracker.score on the COMPLETED table of the latest `run()`: the unchanged air_track_score with T := C on sm_boxes,
        sm_count, sm_id, so a frame a track coasted over counts a match when the filled box is on the object.  gt_boxes [R, G, 4] or
        [S, F, G, 4].  Returns seq_counts [S, 8] int32 (track.COUNTS), seq_iou [S] float64, gt_match [R, G] int32 (the matched ROW)
        and this object's own running totals_i [8] int64 / totals_f [1] float64 (accumulate=False: restarts), all on the device.
        identity=True: air_track_idf behind it (the ids are the tracker's: n_ids = F T), as SequenceTracker.score describes --
        seq_idf, idf_overlap, totals_idf, read by `identity_summary()`."""
        return self.scores.result(self._run_score("completed", gt_boxes, tau, self.F, identity), bool(accumulate))

    def score_forecast(self, gt_future_boxes, tau=0.5, identity=False):
        """the same kernel on the FORECAST table with F := Hz: gt_future_boxes [S Hz, G, 4] or [S, Hz, G, 4], slot g the same object
        over the horizon.  Returns seq_counts [S, 8], seq_iou [S], gt_match [S Hz, G], with identity=True seq_idf [S, 4] and
        idf_overlap [S, G, F T] too; nothing is accumulated."""
        if self.fc is None:
            raise ValueError("score_forecast needs a horizon >= 1; this smoother was built with horizon=0")
        return self.scores.result(self._run_score("forecast", gt_future_boxes, tau, self.horizon, identity))

    def _hota_entry(self, table, G):
        return self.scores.hota_entry((table,), G, self._score_table(table, "air_track_hota"), self.F * self.window_T)

    def hota(self, gt_boxes, accumulate=True):
        """SequenceTracker.hota on the COMPLETED table of the latest `run()`: air_track_hota with T := C on sm_boxes, sm_count, sm_id
        (the ids are the tracker's: n_ids = F T), so a frame a track coasted over and the smoother filled is a detection, no longer a
        miss.  Returns seq_hota_i, seq_hota_f, hota_potential, hota_id_count, hota_gt_count, hota_matches and this object's own
        running totals_hota_i / totals_hota_f (accumulate=False: restarts), all on the device."""
        return self.scores.run_hota(gt_boxes, self.F, lambda G: self._hota_entry("completed", G), bool(accumulate))

    def hota_forecast(self, gt_future_boxes):
        """the same kernel on the FORECAST table with F := Hz, like `score_forecast`; nothing is accumulated"""
        if self.fc is None:
            raise ValueError("hota_forecast needs a horizon >= 1; this smoother was built with horizon=0")
        return self.scores.run_hota(gt_future_boxes, self.horizon, lambda G: self._hota_entry("forecast", G))

    def hota_summary(self) -> Dict[str, object]:
        """track.hota_summary of everything `hota` took since the last reset (ONE read-back)"""
        return self.scores.hota_summary()

    def mots(self, gt_instances, n_slots=MAX_GT, accumulate=True):
        """SequenceTracker.mots on the COMPLETED table of the latest `run()`: the unchanged air_score_contingency of sm_owner (the
        ROW that owns a pixel of the completed frame's rendering) and the instance maps, then air_track_mots with T := C on sm_count
        and sm_id -- so a frame a track coasted over counts a match when the filled mask is on the object.  Returns seq_mots_i,
        seq_mots_f, mots_match (the matched ROW), mots_iou, cont and this object's own running totals_mots_i / totals_mots_f
        (accumulate=False: restarts), all on the device."""
        t = self.sm
        return self.scores.run_mots(gt_instances, ("completed",), n_slots, (self.C, self.F, t["owner"], t["count"], t["id"]),
                                    bool(accumulate))

    def mots_summary(self) -> Dict[str, float]:
        """track.mots_summary of everything `mots` took since the last reset (ONE read-back)"""
        return self.scores.mots_summary()

    def reset(self):
        """zero the totals"""
        self.scores.reset()

    def summary(self) -> Dict[str, float]:
        """track.mot_summary of everything `score` took since the last reset (ONE read-back)"""
        return self.scores.summary()

    def identity_summary(self) -> Dict[str, float]:
        """track.idf_summary of everything `score(identity=True)` took since the last reset (ONE read-back)"""
        return self.scores.identity_summary()


class StreamSmoother(BoundStage):
    """Trajectories on a STREAM: binds to a track.StreamTracker and gives every chunk fixed-lag smoothed, gap-filled rows and a forecast
    (the module text states the rule; include/air_hip.h the layout of the carried state).  A frame is emitted `lag` frames late,
    max_age <= lag <= MAX_LAG, with the bits TrajectorySmoother gives it on the sequence truncated `lag` frames behind it -- whatever the
    chunking; the forecast needs no lag.  `push` is the tracker's `push` and then, after `capture()`, ONE hipGraph: air_track_stash,
    air_track_smooth_stream, air_track_fill_stream and the unchanged read-out kernels on the emitted and on the forecast table.
    `tail()` smooths the frames that are not final yet (the flush at the end of a video) on a plan and graph of its own and leaves
    the state alone.  The tracker's state and the provider's buffers are only read; the smoother keeps a track table, the ring of
    filter values and the ring of provider rows of the last D = chunk_frames + lag + max_age frames of its own, on the device.
    `emitted` is the provider surface of the emitted frames (score.ParseScorer binds to it).  The default lag (max_age) and the noise
    terms are provisional: UNMEASURED on a trained model."""
    KEY_FIELDS = ("output_multiplier", "output_std")

    def __init__(self, stream_tracker, lag=None, horizon=0, process_noise=DEFAULTS["process_noise"],
                 measurement_noise=DEFAULTS["measurement_noise"], velocity_var=DEFAULTS["velocity_var"]):
        import numpy as np
        import torch
        from . import hip as H
        tk = stream_tracker
        if not hasattr(tk, "frames_seen") or not hasattr(tk, "push"):
            raise ValueError("StreamSmoother binds to a track.StreamTracker, got %s" % type(tk).__name__)
        T, F, S, C, L, Hz, D, q, r, vv = check_stream_arguments(tk.T, tk.F, tk.R, tk.max_age, lag, horizon, process_noise,
                                                                measurement_noise, velocity_var)
        provider = tk.provider
        self.tracker, self.provider, self.engine, self.parser, self._bound = tk, provider, tk.engine, provider, tk
        self.window_T, self.T, self.C, self.R, self.S, self.F, self.horizon, self.lag, self.depth = T, C, C, int(tk.R), S, F, Hz, L, D
        self.process_noise, self.measurement_noise, self.velocity_var, self.max_age = q, r, vv, int(tk.max_age)
        self.mask_threshold, self.img_size = provider.mask_threshold, tuple(tk.img_size)
        self._rows = {k: tk._rows[k] for k in ("what", "where", "glimpse")}
        cfg = self.engine.cfg
        self.A, self.G = int(tk.A), int(cfg.crop_size[0]) * int(cfg.crop_size[1])
        dev, R = self.engine.device, self.R
        lib = H.lib()
        self._H = H
        self._layout, self.state_bytes = smooth_state_layout(S, D)
        if int(lib.air_track_smooth_stream_state_bytes(S, D)) != self.state_bytes:
            raise ValueError("a smoother state of %d sequences at depth %d does not fit the kernel's limits" % (S, D))
        bands = lambda N: int(lib.air_canvas_unroll_bands(N, self.img_size[0])) if N else 0
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.packed = z((self.state_bytes,), torch.uint8)
            self.state = {k: self.packed[at:at + int(np.prod(shape)) * np.dtype(dt).itemsize].view(getattr(torch, np.dtype(dt).name))
                          .view(shape) for k, (at, dt, shape) in self._layout.items()}
            self.rings = {"what": z((S, D, T, self.A)), "glimpse": z((S, D, T, self.G)), "score": z((S, D, T))}
            self.score_state = {"score_i": z((S, 32), torch.int32), "score_f": z((S,), torch.float64)}
            (self.sm, self._sm_ro) = self._table(z, R, bands(R))
            (self.fc, self._fc_ro) = self._table(z, S * Hz, bands(S * Hz)) if Hz else (None, None)
            (self.tl, self._tl_ro) = self._table(z, S * L, bands(S * L)) if L else (None, None)
            self.sm_counts, self.emit_frame, self.num_emitted = z((S, 3), torch.int32), z((S, F), torch.int32), z((S,), torch.int32)
            self.tail_frame = z((S, max(L, 1)), torch.int32)
        self.frames_seen = np.zeros(S, np.int64)                   # the host's mirror of state["seq"][:, 0]
        self.scores = IdentityScores(self, S)
        self._score, self._tail = self.scores.entries, {"plan": [], "graph": None}
        t = self.sm
        self.what, self.where, self.glimpse, self.boxes = t["what"], t["where"], t["glimpse"], t["boxes_out"]
        self.presence, self.num_objects, self.owner = t["presence"], t["num_objects"], t["owner"]
        self.emitted = CompletedFrames(self)
        self._rebuild()
        for name in ("readout", "readout_forecast"):
            if name in self.segments:
                self.check_render(self.segments[name][2],
                                  "air_parse_render declines %d x %d frames with %d emitted rows: its LDS carve passes the 160 KiB "
                                  "of a workgroup; use a smaller max_age" % (self.img_size + (self.C,)))
        self._reset_own(np.arange(S))
        self.engine.synchronize()

    _table = TrajectorySmoother._table
    _readout = TrajectorySmoother._readout

    def _fill(self, t, N, per_seq):
        L, p, rg = self._H.lib(), self._H._p, self.rings
        return [(L.air_track_fill_stream,
                 (p(rg["what"]), p(rg["glimpse"]), p(rg["score"]), p(t["state"]), p(t["src_frame"]), p(t["src_slot"]), self.window_T,
                  self.S, self.depth, self.C, N, per_seq, self.A, self.G, p(t["what"]), p(t["glimpse"]), p(t["score"])),
                 "air_track_fill_stream")]

    def _build_plan(self):
        tk, par, rows, rg = self.tracker, self.provider, self._rows, self.rings
        L, p, size = self._H.lib(), self._H._p, ctypes.c_size_t
        Hi, Wi = self.img_size
        sm, fc, tl, Hz = self.sm, self.fc, self.tl, self.horizon
        fcp = lambda k: p(fc[k]) if fc is not None else None
        qs, qc = self.process_noise
        table = lambda t: [p(t[k]) for k in ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity", "count")]
        self.segments = OrderedDict([
            ("stash", [(L.air_track_stash,
                        (p(rows["what"]), p(rows["glimpse"]), p(par.score), p(tk.valid), p(self.packed), self.window_T, self.S, self.F,
                         self.R, self.A, self.G, self.depth, p(rg["what"]), p(rg["glimpse"]), p(rg["score"])), "air_track_stash")]),
            ("smooth", [(L.air_track_smooth_stream,
                         (p(rows["where"]), p(par.num_objects), p(tk.track_id), p(tk.valid), self.window_T, self.S, self.F, self.R,
                          self.C, self.lag, Hz, self.depth, self.max_age, Hi, Wi, qs, qc, self.measurement_noise, self.velocity_var,
                          p(self.packed), size(self.state_bytes), *table(sm), p(self.sm_counts), p(self.emit_frame),
                          p(self.num_emitted), *[fcp(k) for k in ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity",
                                                                   "count")]), "air_track_smooth_stream")]),
            ("fill", self._fill(sm, self.R, self.F)),
            ("readout", self._readout(sm, self._sm_ro))])
        if fc is not None:
            self.segments["fill_forecast"] = self._fill(fc, self.S * Hz, Hz)
            self.segments["readout_forecast"] = self._readout(fc, self._fc_ro)
        self._plan = [e for seg in self.segments.values() for e in seg]
        self._tail["plan"] = [] if tl is None else (
            [(L.air_track_smooth_tail, (self.window_T, self.S, self.C, self.lag, self.depth, self.max_age, Hi, Wi, p(self.packed),
                                        size(self.state_bytes), *table(tl), p(self.tail_frame)), "air_track_smooth_tail")]
            + self._fill(tl, self.S * self.lag, self.lag) + self._readout(tl, self._tl_ro))

    def _score_entries(self):
        return [e for e in list(self._score.values()) + [self._tail] if e["plan"]]

    def launch_count(self) -> Dict[str, int]:
        """entries of one `push()` behind the tracker's own (`tracker` holds that tracker's launch_count()); `tail` those of `tail()`"""
        n = 2 if self.fc is not None else 1
        return {"tracker": self.tracker.launch_count(), "track_stash": 1, "track_smooth_stream": 1, "track_fill_stream": n,
                "parse_objects": n, "tile_relabel": n, "parse_render": n, "tail": len(self._tail["plan"])}

    # ---- the state ----------------------------------------------------------------------------------------------------------------
    def _reset_own(self, rows):
        import torch
        eng, st = self.engine, self.state
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            idx = torch.as_tensor(rows, device=eng.device)
            i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=eng.device)
            st["seq"][idx] = 0
            st["slots"][idx] = i32(SM_EMPTY)[None, :, None].expand(len(rows), 6, MAX_SLOTS)
            st["ring_i"][idx] = i32(RING_EMPTY)[None, None, :, None].expand(len(rows), self.depth, 4, MAX_SLOTS)
            st["ring"][idx] = 0
            for buf in self.rings.values():
                buf[idx] = 0
            self.score_state["score_i"][idx] = 0
            self.score_state["score_i"][idx, 8:16] = -1
            self.score_state["score_f"][idx] = 0
        self.frames_seen[rows] = 0
        eng.wait_for_engine()

    def reset(self, sequences=None):
        """restart all (None) or some sequences ON THE DEVICE: the tracker's state AND the smoother's (its table, rings and score state)"""
        import numpy as np
        rows = np.arange(self.S) if sequences is None else np.atleast_1d(np.asarray(sequences, np.int64))
        self.tracker.reset(sequences)
        self._reset_own(rows)

    def state_dict(self):
        """a copy of everything carried: the tracker's state_dict() under "tracker", the packed smoother state, the rings of provider
        rows and the score state, as plain device tensors"""
        import torch
        out = {"tracker": self.tracker.state_dict()}
        eng = self.engine
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            out["smooth"] = self.packed.clone()
            out.update({"ring_" + k: v.clone() for k, v in self.rings.items()})
            out.update({k: v.clone() for k, v in self.score_state.items()})
        eng.wait_for_engine()
        return out

    def load_state_dict(self, state):
        import torch
        own = dict({"smooth": self.packed}, **{"ring_" + k: v for k, v in self.rings.items()}, **self.score_state)
        for k, buf in own.items():
            if tuple(state[k].shape) != tuple(buf.shape):
                raise ValueError("load_state_dict: %s has shape %s, this stream's is %s" % (k, tuple(state[k].shape), tuple(buf.shape)))
        self.tracker.load_state_dict(state["tracker"])
        eng = self.engine
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            for k, buf in own.items():
                buf.copy_(torch.as_tensor(state[k]).to(buf.dtype), non_blocking=True)
        eng.wait_for_engine()
        eng.synchronize()
        self.frames_seen[:] = self.state["seq"][:, 0].cpu().numpy()

    # ---- the trajectories -------------------------------------------------------------------------------------------------------------
    def _check_mirror(self, fed_limit):
        import numpy as np
        fed = np.asarray(self.tracker.frames_seen, np.int64) - self.frames_seen
        if (fed < 0).any() or (fed > fed_limit).any():
            s = int(np.argmax((fed < 0) | (fed > fed_limit)))
            raise ValueError("the tracker has seen %d frames of sequence %d, the smoother %d: the tracker was reset or pushed behind "
                             "the smoother's back; reset() both through the smoother, or load_state_dict()"
                             % (int(self.tracker.frames_seen[s]), s, int(self.frames_seen[s])))

    def run(self, base=None):
        """the trajectories of the tracker's LATEST push (which the smoother has not seen yet); `base` is passed through"""
        eng = self.engine
        self._check_mirror(self.F)
        self._refresh_plan()
        eng.wait_for_caller()
        eng._replay_or_run(self._graph, self._plan)
        self.frames_seen = self.tracker.frames_seen.copy()
        eng.wait_for_engine()
        return self.result(base)

    def push(self, frames, valid=None, *args, **kwargs):
        """the bound tracker's `push(frames, valid, ...)`, then `run()` on its result.  Refused when the tracker's frames_seen differs
        from the smoother's"""
        self._check_mirror(0)
        return self.run(self.tracker.push(frames, valid, *args, **kwargs))

    def result(self, base=None):
        """TrajectorySmoother.result's tensors for the EMITTED table: sm_* at [C, S F] columns s F + e, emit_frame [S, F] (the global
        frame of column e, -1: none), num_emitted [S]; with a horizon fc_* at [C, S Hz] and frames_pred [S, Hz, H, W]"""
        out = TrajectorySmoother.result(self, base)
        out.update(emit_frame=self.emit_frame, num_emitted=self.num_emitted)
        return out

    def tail(self):
        """the frames max(0, b - lag) .. b - 1, not final yet, smoothed with what is known: tl_* at [C, S lag] columns s lag + j (every
        tensor `result` lists under sm_), tail_frame [S, lag] (-1: none).  Reads the state and changes nothing: the stream goes on"""
        if self.tl is None:
            raise ValueError("lag = 0: every frame is final when it is seen; there is no tail")
        eng = self.engine
        self._refresh_plan()
        eng.wait_for_caller()
        eng._replay_or_run(self._tail["graph"], self._tail["plan"])
        eng.wait_for_engine()
        out = _table_result("tl_", self.tl, self.C, eng.cfg.crop_size)
        out["tail_frame"] = self.tail_frame
        return out

    # ---- the identity metric on the emitted frames ------------------------------------------------------------------------------------
    def score(self, gt_boxes, tau=0.5):
        """StreamTracker.score on the EMITTED table of the latest push: the unchanged air_track_score_stream with T := C and valid :=
        num_emitted on sm_boxes, sm_count, sm_id, continuing CLEAR-MOT across the pushes.  gt_boxes [R, G, 4] or [S, F, G, 4]: row
        s F + e the ground truth of global frame emit_frame[s, e] (the caller keeps it `lag` frames).  Once per push.  Returns
        seq_counts [S, 8], seq_iou [S] float64 (cumulative) and gt_match [R, G] of the emitted columns."""
        sm = self.sm
        return self.scores.run_stream(gt_boxes, tau, (self.C, self.F, sm["boxes"], sm["count"], sm["id"]), self.num_emitted,
                                      self.score_state, "this stream is scored with (G, tau) = %r; a stream of its own for %r",
                                      "gt_boxes: 1..%d ground-truth slots and tau within [0, 1], got %d and %r")

    def summary(self) -> Dict[str, float]:
        """track.mot_summary of the emitted frames scored so far (ONE read-back)"""
        return self.scores.stream_summary()


# ---- the noise terms by maximum likelihood (the module text states the statistics; include/air_hip.h the kernels' order) --------------------
FIT_MAX_CANDIDATES = 32                                            # NFIT_MAX_G: candidates per launch
# the fit's domain (csrc/noise_fit_kernels.hip: NFIT_*): the smoother's supported ratios, so that a fitted setting is one it takes
FIT_Q_OVER_R_MIN, FIT_Q_OVER_R_MAX, FIT_V_OVER_R_MAX = Q_OVER_R_MIN, Q_OVER_R_MAX, V_OVER_R_MAX
DEFAULT_FIT_RATIOS = tuple(float(10.0 ** (0.5 * k)) for k in range(-12, 7))      # half-decades of rho from 1e-6 to 1e3: 19 values
FIT_KEYS = ("process_noise", "measurement_noise", "velocity_var")  # what of a fit `smooth=` takes as it is
TOTAL_KEYS = ("tot_q", "tot_m", "tot_k", "tot_n")


def default_velocity_ratio() -> float:
    return DEFAULTS["velocity_var"] / DEFAULTS["measurement_noise"]


def check_fit_arguments(max_steps, n_frames, n_rows=None, shift_ratios=None, scale_ratios=None, velocity_ratio=None, domain=True):
    """Refuse what air_track_noise_stats refuses (pure host code).  None: DEFAULT_FIT_RATIOS / default_velocity_ratio().  Returns
    (T, F, S, shift_ratios, scale_ratios, velocity_ratio), the ratios as tuples of G floats.  domain=False keeps every check but the
    limits of the ratios (the numpy restatement runs wherever the statements do)."""
    T, F, S = check_track_arguments(max_steps, n_frames, n_rows)
    grids = []
    for name, given in (("shift_ratios", shift_ratios), ("scale_ratios", scale_ratios)):
        try:
            g = tuple(float(v) for v in (DEFAULT_FIT_RATIOS if given is None else given))
        except TypeError:
            raise ValueError("%s must be a sequence of numbers, got %r" % (name, given))
        if not 1 <= len(g) <= FIT_MAX_CANDIDATES:
            raise ValueError("%s must hold 1..%d candidates, got %d" % (name, FIT_MAX_CANDIDATES, len(g)))
        if not all(v > 0.0 for v in g):
            raise ValueError("%s must be positive numbers (process noise / measurement noise), got %r" % (name, g))
        if domain and not all(FIT_Q_OVER_R_MIN <= v <= FIT_Q_OVER_R_MAX for v in g):
            raise ValueError("%s must lie within FIT_Q_OVER_R_MIN..FIT_Q_OVER_R_MAX = %g..%g (the smoother's supported domain), got %r"
                             % (name, FIT_Q_OVER_R_MIN, FIT_Q_OVER_R_MAX, g))
        grids.append(g)
    if len(grids[0]) != len(grids[1]):
        raise ValueError("shift_ratios and scale_ratios must hold the same number of candidates (one launch evaluates candidate g of "
                         "both), got %d and %d" % (len(grids[0]), len(grids[1])))
    nu = default_velocity_ratio() if velocity_ratio is None else float(velocity_ratio)
    if not nu >= 0.0:
        raise ValueError("velocity_ratio must be a number >= 0 (velocity_var / measurement noise), got %r" % (velocity_ratio,))
    if domain and not nu <= FIT_V_OVER_R_MAX:
        raise ValueError("velocity_ratio must be at most FIT_V_OVER_R_MAX = %g (the smoother's supported domain), got %r"
                         % (FIT_V_OVER_R_MAX, velocity_ratio))
    return T, F, S, grids[0], grids[1], nu


def _pair_mul(m, k, ms, ks):
    """(m, k) x (ms, ks) of products kept as m 2^k: (m, j) = frexp(m ms), k += ks + j.  Arrays, elementwise"""
    import numpy as np
    mm, j = np.frexp(m * ms)
    return mm, k + ks + j.astype(np.int64)


def _track_noise_stats(z_of, first, last, rho, nu):
    """the forward filter of one track at r = 1 on every candidate at once: rho [2, G] float64 (class 0 the shifts, 1 the scales),
    z_of(f) -> float64 [4] or None.  Returns Q, m [2, G] float64, k [2, G] int64 and the number of updates.  The statements are
    `_filter_step`'s at r = 1, elementwise over the candidates; per update and class s~ = Pxx- + 1, d = (e_a e_a + e_b e_b) / s~,
    Q = Q + d, (m, k) x frexp(s~)."""
    import numpy as np
    G = rho.shape[1]
    one = np.float64(1.0)
    q, q2, q4 = rho, np.float64(0.5) * rho, np.float64(0.25) * rho
    Q, M, K, n = np.zeros((2, G)), np.full((2, G), 0.5), np.ones((2, G), np.int64), 0
    cls = list(_CLASS)
    x = v = Pxx = Pxv = Pvv = None
    for f in range(first, last + 1):
        z = z_of(f)
        if f == first:                                             # start: x = z, v = 0, P = (1, 0, nu)
            x = np.repeat((np.zeros(4) if z is None else z)[:, None], G, axis=1)
            v, Pxx, Pxv, Pvv = np.zeros((4, G)), np.ones((2, G)), np.zeros((2, G)), np.full((2, G), np.float64(nu))
            continue
        a, b = Pxx + Pxv, Pxv + Pvv
        Pxxp, Pxvp, Pvvp = (a + b) + q4, b + q2, Pvv + q
        xp = x + v
        if z is None:                                              # a coasted frame keeps the predicted state
            x, Pxx, Pxv, Pvv = xp, Pxxp, Pxvp, Pvvp
            continue
        sn = Pxxp + one
        kx, kv = Pxxp / sn, Pxvp / sn
        Pxx, Pxv, Pvv = Pxxp - kx * Pxxp, Pxvp - kx * Pxvp, Pvvp - kv * Pxvp
        e = z[:, None] - xp
        x, v = xp + kx[cls] * e, v + kv[cls] * e
        for c, (ca, cb) in enumerate(((1, 3), (0, 2))):
            Q[c] = Q[c] + (e[ca] * e[ca] + e[cb] * e[cb]) / sn[c]
            ms, ks = np.frexp(sn[c])
            M[c], K[c] = _pair_mul(M[c], K[c], ms, ks.astype(np.int64))
        n += 1
    return Q, M, K, n


def new_noise_totals(n_candidates):
    """totals that hold nothing: the identities 0.0 and (0.5, 1) and n = 0"""
    import numpy as np
    G = int(n_candidates)
    return {"tot_q": np.zeros((G, 2)), "tot_m": np.full((G, 2), 0.5), "tot_k": np.ones((G, 2), np.int64), "tot_n": np.zeros(1, np.int64)}


def reference_noise_reduce(q, m, k, n, totals=None, accumulate=True):
    """air_track_noise_reduce restated: q, m [S, G, 2] float64, k [S, G, 2], n [S] integers combined in ascending s from the
    identities; then written (totals None or accumulate False) or combined into `totals` (total first; it is not modified).
    Returns {tot_q, tot_m [G, 2] float64, tot_k [G, 2] int64, tot_n [1] int64}."""
    import numpy as np
    q, m, k = np.asarray(q, np.float64), np.asarray(m, np.float64), np.asarray(k).astype(np.int64)
    fresh = new_noise_totals(q.shape[1])
    Q, M, K = fresh["tot_q"], fresh["tot_m"], fresh["tot_k"]
    with np.errstate(all="ignore"):
        for s in range(q.shape[0]):
            Q = Q + q[s]
            M, K = _pair_mul(M, K, m[s], k[s])
        N = np.asarray(n).astype(np.int64).sum(keepdims=True).reshape(1)
        if totals is not None and accumulate:
            Q = np.asarray(totals["tot_q"], np.float64) + Q
            M, K = _pair_mul(np.asarray(totals["tot_m"], np.float64), np.asarray(totals["tot_k"]).astype(np.int64), M, K)
            N = np.asarray(totals["tot_n"]).astype(np.int64).reshape(1) + N
    return {"tot_q": Q, "tot_m": M, "tot_k": K, "tot_n": N}


def reference_noise_stats(where, num_objects, track_id, num_tracks, track_first, track_last, n_frames, shift_ratios, scale_ratios,
                          velocity_ratio, totals=None, accumulate=True):
    """air_track_noise_stats and air_track_noise_reduce restated in numpy float64, bit for bit, the combine order included: the tables
    as `reference_smooth` takes them (the same clipping and skip rules), G candidates, the filter at r = 1.  Per sequence and
    candidate the lanes of a pass of 64 ids are combined by a binary tree (strides 32 .. 1, lane i < stride takes lane i + stride, an
    idle lane the identities 0.0 and (0.5, 1)), the passes in ascending order, the sequences in ascending order, then the totals
    (`reference_noise_reduce`: totals / accumulate).  Several calls accumulate by passing the totals of the call before.  Returns
    q, m [S, G, 2] float64, k [S, G, 2] int32, n [S] int32 and tot_q, tot_m, tot_k, tot_n.  The ratios' domain is not checked here."""
    import numpy as np
    where = np.asarray(where, np.float32)
    T, R = where.shape[:2]
    T, F, S, shift, scale, nu = check_fit_arguments(T, n_frames, R, shift_ratios, scale_ratios, velocity_ratio, domain=False)
    G, FT = len(shift), F * T
    rho = np.array([shift, scale], np.float64)
    ids, n_in = np.asarray(track_id).astype(np.int64), np.asarray(num_objects).astype(np.int64)
    first, last = np.asarray(track_first).reshape(S, FT).astype(np.int64), np.asarray(track_last).reshape(S, FT).astype(np.int64)
    out = {"q": np.zeros((S, G, 2)), "m": np.zeros((S, G, 2)), "k": np.zeros((S, G, 2), np.int32), "n": np.zeros(S, np.int32)}
    with np.errstate(all="ignore"):
        for s in range(S):
            issued = int(min(max(int(np.asarray(num_tracks)[s]), 0), FT))

            def sighting(i, f):
                rr = s * F + f
                n = int(min(max(n_in[rr], 0), T))
                return next((j for j in range(n) if ids[j, rr] == i), None)

            Qs, Ms, Ks, Ns = np.zeros((2, G)), np.full((2, G), 0.5), np.ones((2, G), np.int64), 0
            for base in range(0, issued, 64):
                Ql, Ml, Kl = np.zeros((64, 2, G)), np.full((64, 2, G), 0.5), np.ones((64, 2, G), np.int64)
                for lane in range(64):
                    i = base + lane
                    if i >= issued or not 0 <= first[s, i] <= last[s, i] < F:
                        continue
                    fi, la = int(first[s, i]), int(last[s, i])
                    slots = {f: sighting(i, f) for f in range(fi, la + 1)}
                    z_of = lambda f: None if slots[f] is None else where[slots[f], s * F + f].astype(np.float64)
                    Ql[lane], Ml[lane], Kl[lane], n_t = _track_noise_stats(z_of, fi, la, rho, nu)
                    Ns += n_t
                stride = 32
                while stride >= 1:                                 # lane i < stride takes lane i + stride
                    Ql[:stride] = Ql[:stride] + Ql[stride:2 * stride]
                    Ml[:stride], Kl[:stride] = _pair_mul(Ml[:stride], Kl[:stride], Ml[stride:2 * stride], Kl[stride:2 * stride])
                    stride //= 2
                Qs = Qs + Ql[0]                                    # the passes in ascending order
                Ms, Ks = _pair_mul(Ms, Ks, Ml[0], Kl[0])
            out["q"][s], out["m"][s], out["k"][s], out["n"][s] = Qs.T, Ms.T, Ks.T.astype(np.int32), Ns
    out.update(reference_noise_reduce(out["q"], out["m"], out["k"], out["n"], totals, accumulate))
    return out


def _profile_terms(totals):
    """(N, Q [G, G], Lambda [G, G]) of the totals: Q = Q_0(i) + Q_1(j), Lambda = Lambda_0(i) + Lambda_1(j) with
    Lambda_c = 2 (log m + k log 2) -- the two components of a class share every s~ --, N = 4 n"""
    import numpy as np
    tq, tm = np.asarray(totals["tot_q"], np.float64), np.asarray(totals["tot_m"], np.float64)
    tk = np.asarray(totals["tot_k"]).astype(np.float64)
    with np.errstate(all="ignore"):
        lam = 2.0 * (np.log(tm) + tk * np.log(2.0))
    N = 4 * int(np.asarray(totals["tot_n"]).reshape(-1)[0])
    return N, tq[:, 0][:, None] + tq[:, 1][None, :], lam[:, 0][:, None] + lam[:, 1][None, :]


def profile_loglik(totals, i, j, r):
    """loglik(r) = -1/2 [N log(2 pi r) + Lambda + Q / r] of cell (i, j): the value at a GIVEN measurement noise r -- at the current
    settings, say, to compare with a fit's `loglik` on the same tracks"""
    import math
    N, Q, lam = _profile_terms(totals)
    return float(-0.5 * (N * math.log(2.0 * math.pi * float(r)) + lam[i, j] + Q[i, j] / float(r)))


def profile_fit(totals, shift_ratios, scale_ratios, velocity_ratio):
    """The maximum-likelihood noise terms from the totals, host float64.  The G x G profile surface is
    loglik^[i, j] = -1/2 [N (log(2 pi Q / N) + 1) + Lambda], r concentrated out as r^ = Q / N; its arg-max is the FIRST cell in
    row-major order (i: shift, j: scale) that no later cell exceeds, and a NaN never wins.  Returns dict(process_noise=(r^ rho_shift,
    r^ rho_scale), measurement_noise=r^, velocity_var=r^ nu, loglik, n_innovations=N, cell=(i, j), on_edge=(bool, bool), surface
    [G, G]); the first three are what `smooth=` takes.  ValueError: no track with two sightings (n = 0); Q = 0 (every innovation is
    zero: the likelihood is unbounded); no finite cell; fitted terms outside the smoother's supported domain."""
    import numpy as np
    shift, scale = [float(v) for v in shift_ratios], [float(v) for v in scale_ratios]
    nu = float(velocity_ratio)
    N, Q, lam = _profile_terms(totals)
    G = Q.shape[0]
    if len(shift) != G or len(scale) != G:
        raise ValueError("the totals hold %d candidates, the grids %d and %d" % (G, len(shift), len(scale)))
    if N == 0:
        raise ValueError("no track with two sightings: there is no innovation to fit the noise terms to")
    if (Q == 0.0).any():
        raise ValueError("every innovation is zero (the tracks do not move off their prediction): the likelihood is unbounded as the "
                         "measurement noise goes to 0, there is no maximum")
    with np.errstate(all="ignore"):
        surface = -0.5 * (N * (np.log(2.0 * np.pi * Q / N) + 1.0) + lam)
    best = None
    for i in range(G):
        for j in range(G):
            v = surface[i, j]
            if v == v and (best is None or v > surface[best]):
                best = (i, j)
    if best is None:
        raise ValueError("the likelihood is NaN in every cell (a non-finite sighting?)")
    i, j = best
    r = float(Q[i, j] / N)
    fit = dict(process_noise=(r * shift[i], r * scale[j]), measurement_noise=r, velocity_var=r * nu)
    try:
        check_arguments(1, 1, None, 0, 0, **fit)
    except ValueError as e:
        raise ValueError("the fitted terms fall outside the smoother's supported domain (cell %r, r = %g): %s" % (best, r, e))
    fit.update(loglik=float(surface[i, j]), n_innovations=N, cell=best, on_edge=(i in (0, G - 1), j in (0, G - 1)), surface=surface)
    return fit


def zoom_grid(ratios, best):
    """the next grid of a zoom: as many candidates, log-spaced between the two neighbours of candidate `best` (the end of the grid
    where there is none), the incumbent itself kept in place of the candidate nearest to it -- so the best cell stays a cell and the
    likelihood cannot go down"""
    import numpy as np
    ratios = [float(v) for v in ratios]
    G = len(ratios)
    lo, hi = ratios[max(best - 1, 0)], ratios[min(best + 1, G - 1)]
    lo, hi = min(lo, hi), max(lo, hi)
    if G == 1 or not hi > lo:
        return tuple(ratios)
    grid = [float(v) for v in np.geomspace(lo, hi, G)]
    grid[0], grid[-1] = lo, hi                                     # (the ends as they were: inside the domain)
    at = int(np.argmin([abs(np.log(g) - np.log(ratios[best])) for g in grid]))
    grid[at] = ratios[best]
    return tuple(grid)


def fit_with_zoom(evaluate, shift_ratios, scale_ratios, velocity_ratio, zoom=0, totals=None):
    """`profile_fit`, then `zoom` times: both grids replaced by `zoom_grid` around the best cell, evaluate(shift, scale) -> totals on
    the SAME tracks, and the better of the two fits kept.  totals: those of the first grid (None: evaluate them).  The returned dict
    also holds shift_ratios / scale_ratios / velocity_ratio, the grid the fit's cell refers to, and `totals`, that grid's."""
    if isinstance(zoom, bool) or int(zoom) != zoom or int(zoom) < 0:
        raise ValueError("zoom must be an integer >= 0, got %r" % (zoom,))
    shift, scale = tuple(float(v) for v in shift_ratios), tuple(float(v) for v in scale_ratios)
    totals = evaluate(shift, scale) if totals is None else totals
    fit = dict(profile_fit(totals, shift, scale, velocity_ratio), shift_ratios=shift, scale_ratios=scale,
               velocity_ratio=float(velocity_ratio), totals=totals)
    for _ in range(int(zoom)):
        shift, scale = zoom_grid(fit["shift_ratios"], fit["cell"][0]), zoom_grid(fit["scale_ratios"], fit["cell"][1])
        totals = evaluate(shift, scale)
        nxt = dict(profile_fit(totals, shift, scale, velocity_ratio), shift_ratios=shift, scale_ratios=scale,
                   velocity_ratio=float(velocity_ratio), totals=totals)
        if nxt["loglik"] >= fit["loglik"]:
            fit = nxt
    return fit


class TrajectoryNoiseFitter(BoundStage):
    """The smoother's noise terms by maximum likelihood, on the device: binds to a track.SequenceTracker like TrajectorySmoother, only
    reads that tracker's and its provider's buffers, and runs, after `capture()`, ONE hipGraph of two launches:

      air_track_noise_stats    the forward filter at r = 1 on a grid of G candidates per noise class, all tracks of all sequences;
      air_track_noise_reduce   the sequences into device-resident totals (always accumulate = 1: `reset()` writes the identities).

    `run()` returns nothing and reads nothing back, so a fit runs over many batches of videos; `fit()` is ONE read-back and
    `profile_fit`.  fit(zoom=k) re-runs k times on `zoom_grid` around the best cell: eager launches into buffers of their own on the
    tracker's CURRENT tables, so it is refused once more than one `run()` has been accumulated (calibration is offline).  Out of
    scope: fitting on a stream; fitting velocity_ratio jointly (fit twice and compare `loglik`: it is comparable on the same tracks);
    noise terms per sequence; the association defaults."""

    def __init__(self, tracker, shift_ratios=None, scale_ratios=None, velocity_ratio=None):
        import torch
        from . import hip as H
        if not hasattr(tracker, "track_first") or hasattr(tracker, "push"):
            raise ValueError("TrajectoryNoiseFitter binds to a track.SequenceTracker, got %s" % type(tracker).__name__)
        T, F, S, shift, scale, nu = check_fit_arguments(tracker.T, tracker.F, tracker.R, shift_ratios, scale_ratios, velocity_ratio)
        self.tracker, self.provider, self.engine, self._bound = tracker, tracker.provider, tracker.engine, tracker
        self.T, self.F, self.S, self.R, self.G = T, F, S, int(tracker.R), len(shift)
        self.shift_ratios, self.scale_ratios, self.velocity_ratio = shift, scale, nu
        self._where = tracker._rows["where"]
        self._H = H
        dev, G = self.engine.device, self.G
        with torch.cuda.device(dev):
            self.stats = self._stat_buffers(torch, dev)
            self.totals, self._zoom_totals = self._total_buffers(torch, dev), self._total_buffers(torch, dev)
            self._identity = {k: torch.as_tensor(v, device=dev) for k, v in new_noise_totals(G).items()}
        self._grid = self._host_grid(shift, scale)
        self.runs = 0
        self._rebuild()
        self.reset()
        self.engine.synchronize()

    def _stat_buffers(self, torch, dev):
        S, G = self.S, self.G
        return {"q": torch.zeros((S, G, 2), dtype=torch.float64, device=dev), "m": torch.zeros((S, G, 2), dtype=torch.float64, device=dev),
                "k": torch.zeros((S, G, 2), dtype=torch.int32, device=dev), "n": torch.zeros((S,), dtype=torch.int32, device=dev)}

    def _total_buffers(self, torch, dev):
        G = self.G
        return {"tot_q": torch.zeros((G, 2), dtype=torch.float64, device=dev), "tot_m": torch.zeros((G, 2), dtype=torch.float64, device=dev),
                "tot_k": torch.zeros((G, 2), dtype=torch.int64, device=dev), "tot_n": torch.zeros((1,), dtype=torch.int64, device=dev)}

    @staticmethod
    def _host_grid(shift, scale):
        """the host arrays the entry copies into the kernel arguments (kept alive by whoever holds the plan)"""
        arr = ctypes.c_double * len(shift)
        return arr(*shift), arr(*scale)

    def _entries(self, grid, totals, accumulate):
        H, tk, par, st = self._H, self.tracker, self.provider, self.stats
        L, p = H.lib(), H._p
        return [(L.air_track_noise_stats,
                 (p(self._where), p(par.num_objects), p(tk.track_id), p(tk.num_tracks), p(tk.track_first), p(tk.track_last), self.T,
                  self.S, self.F, self.R, self.G, grid[0], grid[1], self.velocity_ratio, p(st["q"]), p(st["m"]), p(st["k"]),
                  p(st["n"])), "air_track_noise_stats"),
                (L.air_track_noise_reduce,
                 (p(st["q"]), p(st["m"]), p(st["k"]), p(st["n"]), self.S, self.G, int(accumulate), p(totals["tot_q"]),
                  p(totals["tot_m"]), p(totals["tot_k"]), p(totals["tot_n"])), "air_track_noise_reduce")]

    def _build_plan(self):
        self.segments = OrderedDict([("fit", self._entries(self._grid, self.totals, 1))])
        self._plan = list(self.segments["fit"])

    def launch_count(self) -> Dict[str, int]:
        """entries of one `run()` behind the tracker's own"""
        return {"tracker": self.tracker.launch_count(), "track_noise_stats": 1, "track_noise_reduce": 1}

    def reset(self):
        """the totals hold nothing: the identities 0.0, (0.5, 1) and n = 0, written on the engine's stream"""
        import torch
        eng = self.engine
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            for k, v in self._identity.items():
                self.totals[k].copy_(v, non_blocking=True)
        eng.wait_for_engine()
        self.runs = 0

    def run(self, accumulate=True):
        """the statistics of the tracker's LATEST `track()` into the totals (accumulate=False: `reset()` first).  Returns nothing: no
        read-back.  The tracker's and the provider's buffers are only read.  Same stream contract as SequenceTracker.track."""
        if not accumulate:
            self.reset()
        eng = self.engine
        self._refresh_plan()
        eng.wait_for_caller()
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        self.runs += 1

    def track(self, frames, *args, accumulate=True, **kwargs):
        """the bound tracker's `track(frames, ...)`, then `run(accumulate)`; returns the tracker's result"""
        base = self.tracker.track(frames, *args, **kwargs)
        self.run(accumulate)
        return base

    def read_totals(self, totals=None):
        """{tot_q, tot_m, tot_k, tot_n} as numpy arrays: ONE read-back"""
        import torch
        t = self.totals if totals is None else totals
        self.engine.wait_for_engine()
        flat = torch.cat([t["tot_q"].reshape(-1).view(torch.int64), t["tot_m"].reshape(-1).view(torch.int64), t["tot_k"].reshape(-1),
                          t["tot_n"]]).cpu().numpy()             # (the float64 bits travel as integers)
        G2 = 2 * self.G
        import numpy as np
        return {"tot_q": flat[:G2].view(np.float64).reshape(self.G, 2).copy(), "tot_m": flat[G2:2 * G2].view(np.float64).reshape(self.G, 2).copy(),
                "tot_k": flat[2 * G2:3 * G2].reshape(self.G, 2).copy(), "tot_n": flat[3 * G2:].copy()}

    def _evaluate(self, shift, scale):
        """eager: the two launches on another grid of G candidates into the zoom's own totals (the tracker's current tables)"""
        check_fit_arguments(self.T, self.F, self.R, shift, scale, self.velocity_ratio)
        eng = self.engine
        grid = self._host_grid(shift, scale)
        eng.wait_for_caller()
        eng._run(self._entries(grid, self._zoom_totals, 0), eng._sp())
        eng.wait_for_engine()
        return self.read_totals(self._zoom_totals)

    def fit(self, zoom=0):
        """`profile_fit` of everything `run()` took since the last reset (ONE read-back); zoom=k: `fit_with_zoom`, k eager re-runs on
        the tracker's current tables -- refused when the totals hold more than that one `run()`"""
        if int(zoom) > 0 and self.runs != 1:
            raise ValueError("fit(zoom=%r) re-runs on the tracker's current tables, but the totals hold %d runs: zoom after exactly one "
                             "run() since reset()" % (zoom, self.runs))
        return fit_with_zoom(self._evaluate, self.shift_ratios, self.scale_ratios, self.velocity_ratio, zoom, self.read_totals())
