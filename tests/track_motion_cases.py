"""Cases shared by test_track_motion_host.py and test_track_motion.py: the scenarios of motion-predicted association written as `where`
rows (no model needed), random tracks with gaps, the planted defects of the reference, and the smoother on a tracker's own truncated
output (exact consequence 2)."""
import contextlib

import numpy as np

from attend_infer_repeat_amd import track, trajectory
from attend_infer_repeat_amd.tile import scene_boxes

IMG = (50, 50)
KW = dict(iou_gate=0.1, appearance_weight=0.0)                     # the issue's settings: greedy or optimal, default noise terms
MARGIN = 1e-9
OUTPUTS = ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot", "num_tracks", "track_first", "track_last", "track_length",
           "track_gaps", "state_counts")
MOTION_OUTPUTS = OUTPUTS + ("pred_where", "pred_boxes")
# two corners of the supported noise domain next to the defaults; r is a power of two, so the ratios q / r and velocity_var / r are the
# domain's bounds exactly: the least q / r with no prior rate, and the largest q_shift / r with the largest velocity_var / r
_R = 2.0 ** -11
NOISE = {"defaults": dict(),
         "stiff": dict(process_noise=(_R * trajectory.Q_OVER_R_MIN, _R * trajectory.Q_OVER_R_MIN), measurement_noise=_R, velocity_var=0.0),
         "loose": dict(process_noise=(_R * trajectory.Q_OVER_R_MAX, _R), measurement_noise=_R,
                       velocity_var=_R * trajectory.V_OVER_R_MAX)}


def rows_from_where(objects, F, T, A=2, S=1, img=IMG):
    """provider rows of S identical sequences from `objects`: a list of functions f -> where row [sx, tx, sy, ty] or None (no object in
    that frame).  Object g takes slot (number of objects before it that are present); boxes = scene_boxes(where), score 0.9, what 0;
    gt [R, G, 4]: the box of object g, zero where it is absent."""
    R, G = S * F, len(objects)
    what, where, score = np.zeros((T, R, A), np.float32), np.zeros((T, R, 4), np.float32), np.zeros((T, R), np.float32)
    n, gt = np.zeros(R, np.int32), np.zeros((R, G, 4), np.float32)
    for r in range(R):
        j = 0
        for g, obj in enumerate(objects):
            row = obj(r % F)
            if row is None:
                continue
            where[j, r], score[j, r] = np.asarray(row, np.float32), 0.9
            gt[r, g] = scene_boxes(where[j, r], img)
            j += 1
        n[r] = j
    boxes = scene_boxes(where, img) * (np.arange(T)[:, None, None] < n[None, :, None])
    return dict(what=what, where=where, boxes=boxes.astype(np.float32), score=score, n=n, gt=gt, T=T, A=A, S=S, F=F, img=img)


_obj = lambda tx, gone=(): (lambda f: None if f in gone else (0.2, tx(f), 0.2, 0.0))
# 6 px per frame on the 50 px canvas with 10 px boxes, unseen in frames 4 and 5: the last box (frame 3) no longer reaches frame 6
OCCLUSION = dict(objects=[_obj(lambda f: -0.6 + 0.24 * f, gone=(4, 5))], F=8, T=1, max_age=2,
                 ids=[[0], [0], [0], [0], [], [], [0], [0]], ids_last_box=[[0], [0], [0], [0], [], [], [1], [1]])
# two objects pass through each other; in frame 3 each track's last box lies on the OTHER object
CROSSING = dict(objects=[_obj(lambda f: -0.5 + 0.2 * f), _obj(lambda f: 0.5 - 0.2 * f)], F=6, T=2, max_age=1,
                ids=[[0, 1]] * 6, ids_last_box=[[0, 1]] * 3 + [[1, 0]] * 3)
STATIC = dict(objects=[_obj(lambda f: -0.4), _obj(lambda f: 0.3, gone=(2,))], F=5, T=2, max_age=1)
# displaced by 15 px > its 10 px box in the first step: v = 0 until the second sighting, so neither rule links it
FAST = dict(objects=[_obj(lambda f: -0.6 + 0.6 * f)], F=3, T=1, max_age=1, ids=[[0], [1], [2]])


def scenario(spec, S=1):
    return rows_from_where(spec["objects"], spec["F"], spec["T"], S=S)


def frame_ids(case, out):
    """the track ids of the present objects, per frame of sequence 0"""
    return [[int(out["track_id"][j, f]) for j in range(int(case["n"][f]))] for f in range(case["F"])]


def associate_motion(case, **kw):
    return track.reference_associate_motion(case["what"], case["where"], case["boxes"], case["score"], case["n"], case["F"], case["img"],
                                            **kw)


def associate_last_box(case, **kw):
    return track.reference_associate(case["what"], case["boxes"], case["score"], case["n"], case["F"], **kw)


def random_case(T, A, S, F, seed, max_age=1, matching="greedy", noise=None, static=False, drop=0.25, bad=True, **kw):
    """Random provider rows whose boxes are the scene boxes of their `where` rows: per sequence a few objects that move at a constant
    rate with jitter (static: no rate, no jitter, no clutter and the objects apart -- every sighting of a track carries one value),
    dropouts that last up to max_age frames and longer, clutter, a shuffled slot order, and (bad) non-finite entries in what / where /
    boxes / score and counts outside 0..T.  Redrawn until every IoU is at least MARGIN from the gate and every greedy round is decided
    by at least MARGIN under the motion rule (static: the gate margin alone, under the last-box rule too).  Returns the case and
    reference_associate_motion's answer."""
    R = S * F
    rule = dict(kw, max_age=max_age, matching=matching)
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        what, where = rng.normal(size=(T, R, A)).astype(np.float32), rng.uniform(-1, 1, (T, R, 4)).astype(np.float32)
        score, n = rng.uniform(size=(T, R)).astype(np.float32), np.zeros(R, np.int32)
        for s in range(S):
            k = int(rng.integers(min(T, 3), min(T, 6) + 1))
            pos, vel = rng.uniform(-0.7, 0.7, (k, 2)), rng.uniform(-0.08, 0.08, (k, 2)) * (0 if static else 1)
            size, code = rng.uniform(0.15, 0.35, (k, 2)), rng.normal(size=(k, A))
            if static:                                             # apart, so that no track is ever continued by another object:
                cells = rng.permutation(6)[:k]                     # a 3 x 2 grid of pitch 0.6 > the largest size
                pos = np.stack([-0.6 + 0.6 * (cells % 3), -0.3 + 0.6 * (cells // 3)], -1) + rng.uniform(-0.05, 0.05, (k, 2))
            gone = np.zeros(k, np.int64)                           # frames an object stays unseen from here on
            for f in range(F):
                r, objs = s * F + f, []
                for o in range(k):
                    if gone[o] == 0 and f > 0 and rng.uniform() < drop:
                        gone[o] = rng.integers(1, max_age + 3)
                    if gone[o] > 0:
                        gone[o] -= 1
                        continue
                    jit = 0.0 if static else 1.0
                    c = pos[o] + f * vel[o] + rng.normal(size=2) * 0.01 * jit
                    sz = size[o] + rng.normal(size=2) * 0.005 * jit
                    objs.append(((sz[0], c[0], sz[1], c[1]), rng.uniform(0.3, 1.0), code[o] + rng.normal(size=A) * 0.05 * jit))
                while not static and rng.uniform() < 0.25:         # clutter
                    objs.append(((rng.uniform(0.1, 0.3), rng.uniform(-1, 1), rng.uniform(0.1, 0.3), rng.uniform(-1, 1)), rng.uniform(),
                                 rng.normal(size=A)))
                objs = [objs[i] for i in rng.permutation(len(objs))][:T]
                for j, o in enumerate(objs):
                    where[j, r], score[j, r], what[j, r] = o
                n[r] = len(objs)
                if bad and len(objs) == T and rng.uniform() < 0.3:
                    n[r] = T + 2                                   # clipped to T
        boxes = scene_boxes(where, IMG).astype(np.float32)
        if bad:
            for r in range(R):
                for j in range(int(min(max(n[r], 0), T))):
                    u = rng.uniform()
                    if u < 0.02:
                        boxes[j, r, rng.integers(4)] = rng.choice([np.nan, np.inf, -np.inf])
                    elif u < 0.04:
                        score[j, r] = rng.choice([np.nan, np.inf])
                    elif u < 0.06:
                        what[j, r, rng.integers(A)] = rng.choice([np.nan, -np.inf])
                    elif u < 0.08:
                        where[j, r, rng.integers(4)] = rng.choice([np.nan, np.inf])      # (the box keeps its finite values)
        case = dict(what=what, where=where, boxes=boxes, score=score, n=n, T=T, A=A, S=S, F=F, img=IMG, kw=dict(rule, **(noise or {})))
        refs = [associate_motion(case, return_margins=True, **case["kw"])]
        if static:
            refs.append(associate_last_box(case, return_margins=True, **rule))
        # (static: every track sits on its object with aff = 1 exactly, an exact tie that the ids decide under either rule)
        if all((q["gate_margin"] >= MARGIN).all() and (static or (q.get("round_margin", np.full(S, np.inf)) >= MARGIN).all())
               for q in refs):
            return case, refs[0]
    raise AssertionError("no random case within the margins")


def full_table_case(A=8, F=3, matching="greedy"):
    """T = 32: 32 objects on a grid that drift together, so all 32 slots are live after frame 0 and every one of them is matched in
    each later frame -- every lane advances its filter"""
    T = 32
    objects = [(lambda f, g=g: (0.1, -0.875 + 0.25 * (g % 8) + 0.01 * f, 0.1, -0.6 + 0.4 * (g // 8) + 0.005 * f)) for g in range(T)]
    case = rows_from_where(objects, F, T, A=A)
    case["what"] = np.random.default_rng(5).normal(size=case["what"].shape).astype(np.float32)
    case["kw"] = dict(iou_gate=0.1, appearance_weight=0.25, matching=matching)      # (the random `what` rows keep the affs apart)
    return case


# ---- the planted defects of the reference ----------------------------------------------------------------------------------------------
DEFECTS = ("mv_in_the_advance", "scales_extrapolated", "no_update_after_a_coast", "last_box_for_the_prediction")


@contextlib.contextmanager
def planted(defect):
    """track.reference_associate_motion with one statement of the rule replaced (None: the rule itself)"""
    predict, advance = track._motion_predict, track._motion_advance

    def bad_predict(filt, m, last_box, img_size):
        if defect == "last_box_for_the_prediction":
            return predict(filt, m, last_box, img_size)[0], last_box.copy()
        x, v = filt[0], filt[1]
        pred_where = (x + np.float64(m) * v).astype(np.float32)    # scales_extrapolated
        return pred_where, scene_boxes(pred_where, img_size)

    def bad_advance(filt, m, z, q, r):
        if defect == "no_update_after_a_coast":
            return advance(filt, m, z if m == 1 else None, q, r)
        x, v, Pxx, Pxv, Pvv = filt                                 # mv_in_the_advance: the coasted frames in one product
        cov = (x, v, Pxx, Pxv, Pvv)
        for _ in range(m - 1):
            cov = trajectory._filter_step(cov, None, q, r)[1]
        return trajectory._filter_step((x + np.float64(m - 1) * v, v) + cov[2:], z, q, r)[1]

    if defect in ("scales_extrapolated", "last_box_for_the_prediction"):
        track._motion_predict = bad_predict
    elif defect in ("mv_in_the_advance", "no_update_after_a_coast"):
        track._motion_advance = bad_advance
    else:
        assert defect is None, defect
    try:
        yield
    finally:
        track._motion_predict, track._motion_advance = predict, advance


# ---- exact consequence 2: the smoother on the tracker's own output, truncated -------------------------------------------------------------
def smoother_forecasts(case, out, max_age, noise=None):
    """For every MATCHED object (j, r): (pred_where of the tracker, the fc_where row of its track, column k = 1, of
    trajectory.reference_smooth(horizon=1) on the tracker's output restricted to the frames 0 .. f - 1 of its sequence: track_last
    recomputed from track_id, num_tracks = the ids issued before f)."""
    T, S, F = case["T"], case["S"], case["F"]
    pairs = []
    for s in range(S):
        for f in range(1, F):
            cols = slice(s * F, s * F + f)
            ids, n = out["track_id"][:, cols], np.clip(case["n"][cols], 0, T)
            seen = [(int(ids[j, c]), c) for c in range(f) for j in range(int(n[c])) if ids[j, c] >= 0]
            issued = 1 + max((i for i, _ in seen), default=-1)
            first, last = np.full((1, f * T), -1, np.int32), np.full((1, f * T), -1, np.int32)
            for i, c in seen:
                first[0, i] = c if first[0, i] < 0 else first[0, i]
                last[0, i] = c
            sm = trajectory.reference_smooth(case["where"][:, cols], case["n"][cols], ids, [issued], first, last, f, max_age, case["img"],
                                             horizon=1, **(noise or {}))
            r = s * F + f
            for j in range(int(np.clip(case["n"][r], 0, T))):
                if out["obj_state"][j, r] != track.MATCHED:
                    continue
                row = np.flatnonzero(sm["fc_id"][:, 0] == out["track_id"][j, r])
                assert row.size == 1, (s, f, j)
                pairs.append((out["pred_where"][j, r], sm["fc_where"][row[0], 0]))
    return pairs


def final_states(case, out, max_age, noise=None):
    """(s, id) -> the filtered (x, v) at the last sighting that trajectory._smooth_track gives on the tracker's own complete output"""
    T, S, F = case["T"], case["S"], case["F"]
    terms = dict(trajectory.DEFAULTS, **(noise or {}))
    (q_shift, q_scale), r, vv = terms["process_noise"], terms["measurement_noise"], terms["velocity_var"]
    q = np.array([q_scale, q_shift, q_scale, q_shift], np.float64)
    states = {}
    for s in range(S):
        for i in range(int(out["num_tracks"][s])):
            fi, la = int(out["track_first"][s, i]), int(out["track_last"][s, i])
            slots = {}
            for f in range(fi, la + 1):
                hit = [j for j in range(int(np.clip(case["n"][s * F + f], 0, T))) if out["track_id"][j, s * F + f] == i]
                slots[f] = hit[0] if hit else None
            z_of = lambda f: None if slots[f] is None else case["where"][slots[f], s * F + f].astype(np.float64)
            with np.errstate(all="ignore"):
                states[(s, i)] = trajectory._smooth_track(z_of, fi, la, q, r, vv)[2]
    return states
