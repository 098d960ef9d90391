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
says what was measured).  Out of scope: smoothed covariances, feeding the smoothed rows back into the association, rates on scales in
the forecast, a learned motion prior, particle providers (refused by the tracker, in its wording).
"""
import ctypes
from collections import OrderedDict
from typing import Dict

from .stage import BoundStage, ReadOut, compacted_rows
from .track import MAX_IDS, MAX_SLOTS, IdentityScores
from .track import check_arguments as check_track_arguments

MAX_HORIZON = 16
ABSENT, OBSERVED, FILLED, FORECAST = range(4)
STATES = ("absent", "observed", "filled", "forecast")
DEFAULTS = dict(process_noise=(1e-4, 1e-4), measurement_noise=4e-4, velocity_var=0.04)


def completed_rows(max_steps, max_age) -> int:
    """C = min(32, T (max_age + 1)): a track that spans a frame without a sighting there was last seen in one of the max_age frames
    before it, and the live table holds at most 32 tracks"""
    return min(MAX_SLOTS, int(max_steps) * (int(max_age) + 1))


def check_arguments(max_steps, n_frames, n_rows=None, max_age=1, horizon=0, process_noise=DEFAULTS["process_noise"],
                    measurement_noise=DEFAULTS["measurement_noise"], velocity_var=DEFAULTS["velocity_var"]):
    """Refuse what air_track_smooth refuses (pure host code).  Returns (T, F, S, C, Hz, (q_shift, q_scale), r, velocity_var)."""
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
    if isinstance(horizon, bool) or int(horizon) != horizon or not 0 <= int(horizon) <= MAX_HORIZON:
        raise ValueError("horizon must be an integer within 0..%d, got %r" % (MAX_HORIZON, horizon))
    return T, F, S, completed_rows(T, max_age), int(horizon), q, r, vv


def _smooth_track(z_of, first, last, q, r, vv):
    """the filter and the backward pass of one track: z_of(f) -> float64 [4] or None.  Returns xs, vs {f: [4]}, the filtered (x, v)
    at `last`, and the (frame, value) of every sighting"""
    import numpy as np
    q2, q4 = 0.5 * q, 0.25 * q
    filt, pred = {}, {}
    x = v = Pxx = Pxv = Pvv = None
    for f in range(first, last + 1):
        z = z_of(f)
        if f == first:
            x = np.zeros(4) if z is None else z.copy()
            v, Pxx, Pxv, Pvv = np.zeros(4), np.full(4, r), np.zeros(4), np.full(4, vv)
        else:
            a, b = Pxx + Pxv, Pxv + Pvv
            xp, vp = x + v, v
            Pxxp, Pxvp, Pvvp = (a + b) + q4, b + q2, Pvv + q
            pred[f] = (xp, vp, Pxxp, Pxvp, Pvvp)
            if z is not None:
                s = Pxxp + r
                kx, kv = Pxxp / s, Pxvp / s
                e = z - xp
                x, v = xp + kx * e, vp + kv * e
                Pxx, Pxv, Pvv = Pxxp - kx * Pxxp, Pxvp - kx * Pxvp, Pvvp - kv * Pxvp
            else:
                x, v, Pxx, Pxv, Pvv = xp, vp, Pxxp, Pxvp, Pvvp
        filt[f] = (x, v, Pxx, Pxv, Pvv)
    xs, vs = {last: x}, {last: v}
    for f in range(last - 1, first - 1, -1):
        fx, fv, Pxx, Pxv, Pvv = filt[f]
        xp, vp, Pxxp, Pxvp, Pvvp = pred[f + 1]
        g00, g01, g10, g11 = Pxx + Pxv, Pxv, Pxv + Pvv, Pvv
        det = Pxxp * Pvvp - Pxvp * Pxvp
        C00, C01 = (g00 * Pvvp - g01 * Pxvp) / det, (g01 * Pxxp - g00 * Pxvp) / det
        C10, C11 = (g10 * Pvvp - g11 * Pxvp) / det, (g11 * Pxxp - g10 * Pxvp) / det
        dx, dv = xs[f + 1] - xp, vs[f + 1] - vp
        xs[f] = fx + (C00 * dx + C01 * dv)
        vs[f] = fv + (C10 * dx + C11 * dv)
    return xs, vs, (x, v)


def reference_smooth(where, num_objects, track_id, num_tracks, track_first, track_last, n_frames, max_age, img_size, horizon=0,
                     process_noise=DEFAULTS["process_noise"], measurement_noise=DEFAULTS["measurement_noise"],
                     velocity_var=DEFAULTS["velocity_var"], what=None, glimpse=None, score=None):
    """air_track_smooth (and, with what [T, R, A], glimpse [T, R, G] and score [T, R] given, air_track_fill) restated in numpy float64.
    where [T, R, 4] fp32, num_objects [R], track_id [T, R], num_tracks [S], track_first / track_last [S, F T], R = S n_frames.
    Returns sm_where, sm_boxes [C, R, 4] float32, sm_id [C, R] int32, sm_state [C, R] int8, sm_src_frame, sm_src_slot [C, R] int32,
    sm_velocity [C, R, 2] float32, sm_count [R], sm_counts [S, 3] int32, the same with fc_ and [C, S Hz] for the forecast table
    (fc_count [S Hz]), and sm_what / sm_glimpse / sm_score / fc_what / fc_glimpse / fc_score when the rows to copy are given."""
    import numpy as np
    from .tile import scene_boxes
    where = np.asarray(where, np.float32)
    T, R = where.shape[:2]
    T, F, S, C, Hz, (q_shift, q_scale), r, vv = check_arguments(T, n_frames, R, max_age, horizon, process_noise, measurement_noise,
                                                                velocity_var)
    H, W = (int(v) for v in img_size)
    ids, n_in = np.asarray(track_id).astype(np.int64), np.asarray(num_objects).astype(np.int64)
    FT, N = F * T, S * Hz
    first, last = np.asarray(track_first).reshape(S, FT).astype(np.int64), np.asarray(track_last).reshape(S, FT).astype(np.int64)
    q = np.array([q_scale, q_shift, q_scale, q_shift], np.float64)
    out = {}
    for pre, cols in (("sm_", R), ("fc_", N)):
        out.update({pre + "where": np.zeros((C, cols, 4), np.float32), pre + "boxes": np.zeros((C, cols, 4), np.float32),
                    pre + "id": np.full((C, cols), -1, np.int32), pre + "state": np.zeros((C, cols), np.int8),
                    pre + "src_frame": np.full((C, cols), -1, np.int32), pre + "src_slot": np.full((C, cols), -1, np.int32),
                    pre + "velocity": np.zeros((C, cols, 2), np.float32), pre + "count": np.zeros(cols, np.int32)})
    out["sm_counts"] = np.zeros((S, 3), np.int32)
    half = np.float64(0.5)
    velocity = lambda v: np.array([(np.float64(W) * v[1]) * half, (np.float64(H) * v[3]) * half]).astype(np.float32)

    def put(pre, row, col, w32, vel, tid, state, src):
        out[pre + "where"][row, col], out[pre + "boxes"][row, col] = w32, scene_boxes(w32, (H, W))
        out[pre + "velocity"][row, col], out[pre + "id"][row, col], out[pre + "state"][row, col] = vel, tid, state
        out[pre + "src_frame"][row, col], out[pre + "src_slot"][row, col] = src
        out[pre + "count"][col] = max(out[pre + "count"][col], row + 1)

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
                        m = np.float64(F - 1 - la + k)
                        w32 = np.array([xl[0], xl[1] + m * vl[1], xl[2], xl[3] + m * vl[3]]).astype(np.float32)
                        put("fc_", row, s * Hz + (k - 1), w32, velocity(vl), i, FORECAST, src)
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
        return self._score.values()

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
            if t is None:
                continue
            N = t["count"].shape[0]
            for k in ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity", "count", "what", "score", "presence",
                      "offsets", "obj_image", "obj_step", "obj_box", "obj_score", "obj_where", "obj_what", "reconstruction", "owner",
                      "area"):
                out[pre + k] = t[k]
            out[pre + "glimpse"] = t["glimpse"].view(self.C, N, *cfg.crop_size)
        out["sm_counts"] = self.sm_counts
        if self.fc is not None:
            out["frames_pred"] = self.fc["reconstruction"].view(self.S, self.horizon, *self.img_size)
        return out

    # ---- the identity metric on the tables ------------------------------------------------------------------------------------
    def _score_entry(self, table, G, tau, identity=False):
        t, n_frames = (self.sm, self.F) if table == "completed" else (self.fc, self.horizon)
        if n_frames * self.C > MAX_IDS:
            raise ValueError("air_track_score takes at most %d rows per sequence; %d frames of %d completed rows are %d"
                             % (MAX_IDS, n_frames, self.C, n_frames * self.C))
        return self.scores.entry((table,), G, tau, self.C, n_frames, t["boxes"], t["count"], t["id"], identity, self.F * self.window_T)

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

    def reset(self):
        """zero the totals"""
        self.scores.reset()

    def summary(self) -> Dict[str, float]:
        """track.mot_summary of everything `score` took since the last reset (ONE read-back)"""
        return self.scores.summary()

    def identity_summary(self) -> Dict[str, float]:
        """track.idf_summary of everything `score(identity=True)` took since the last reset (ONE read-back)"""
        return self.scores.identity_summary()
