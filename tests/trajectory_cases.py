"""Cases shared by test_trajectory_host.py and test_trajectory.py: provider rows with the tracker's answer on them (track.reference_associate
on air_parse_objects' boxes of the planted `where` rows, so every table is what a tracker would have written), the planted linear
sequences of the identity figures, and an independent matrix-form smoother."""
import numpy as np

from attend_infer_repeat_amd import track, trajectory
from attend_infer_repeat_amd.tile import scene_boxes

IMG = (50, 50)                                                     # (H, W)
TRACKER_KEYS = ("track_id", "num_tracks", "track_first", "track_last")


def rows_from_objects(frames, T, A, G, seed=0):
    """provider rows from a list, per row r = s F + f, of objects (where [4], score, code): where [T, R, 4], what [T, R, A], glimpse
    [T, R, G], score [T, R] fp32, num_objects [R] int32; what and glimpse are a deterministic fingerprint of the code"""
    R = len(frames)
    rng = np.random.default_rng(seed)
    where, what, glimpse = np.zeros((T, R, 4), np.float32), np.zeros((T, R, A), np.float32), np.zeros((T, R, G), np.float32)
    score, n = np.zeros((T, R), np.float32), np.zeros(R, np.int32)
    for r, objs in enumerate(frames):
        assert len(objs) <= T
        for j, (w, sc, code) in enumerate(objs):
            where[j, r], score[j, r] = w, sc
            what[j, r] = code + 0.01 * rng.normal(size=A)
            glimpse[j, r] = rng.uniform(size=G) + code
        n[r] = len(objs)
    return dict(where=where, what=what, glimpse=glimpse, score=score, n=n)


def with_tracker(rows, F, max_age, img=IMG, **kw):
    """the rows and what a tracker writes on them"""
    boxes = scene_boxes(rows["where"], img)
    ref = track.reference_associate(rows["what"], boxes, rows["score"], rows["n"], F, max_age=max_age, **kw)
    case = dict(rows)
    case.update({k: ref[k] for k in TRACKER_KEYS})
    T, R = rows["score"].shape
    case.update(T=T, R=R, F=F, S=R // F, max_age=max_age, img=img, A=rows["what"].shape[2], G=rows["glimpse"].shape[2], boxes=boxes,
                track_gaps=ref["track_gaps"], track_length=ref["track_length"])
    return case


def drifting_case(T, F, S, max_age, A=5, G=16, seed=0, dropout=0.25, born_last=True):
    """per sequence up to T objects on well separated lanes that drift with jitter, dropouts (gaps of every length, so tracks coast,
    die and are born again), scale wobble, and an object that appears in the last frame only"""
    rng = np.random.default_rng(seed)
    frames = []
    for s in range(S):
        k = T - 1 if (born_last and T > 1) else T
        lane = rng.permutation(T)[:k]
        tx0, vx = rng.uniform(-0.5, 0.1, k), rng.uniform(0.0, 0.06, k)
        for f in range(F):
            objs = []
            for o in range(k):
                if f and rng.uniform() < dropout:
                    continue
                ty = -0.8 + 1.6 * (lane[o] + 0.5) / T
                sx = 0.8 / T * (1.0 + 0.05 * rng.normal())
                objs.append(((sx, tx0[o] + f * vx[o] + 0.003 * rng.normal(), 0.8 / T, ty + 0.002 * rng.normal()), 0.9, float(lane[o])))
            if born_last and T > 1 and f == F - 1:
                free = [l for l in range(T) if l not in lane][0]
                objs.append(((0.8 / T, 0.3, 0.8 / T, -0.8 + 1.6 * (free + 0.5) / T), 0.9, float(free)))
            objs = [objs[i] for i in rng.permutation(len(objs))]
            frames.append(objs)
    return with_tracker(rows_from_objects(frames, T, A, G, seed), F, max_age, iou_gate=0.05)


def jumping_case(T=3, F=24, A=4, G=8, seed=3):
    """every object jumps past the gate in every frame: F T ids of one sighting each, more ids than one pass of lanes"""
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(F):
        side = (-0.6, 0.0, 0.6)[f % 3]                             # (max_age = 1: a place is free again after two frames)
        frames.append([((0.2, side + 0.01 * rng.normal(), 0.2, -0.6 + 0.6 * o), 0.9, float(o)) for o in range(T)])
    case = with_tracker(rows_from_objects(frames, T, A, G, seed), F, 1, iou_gate=0.05)
    assert case["num_tracks"].tolist() == [F * T] and (case["track_first"][0] == case["track_last"][0]).all()
    return case


def full_table_case(A=3, G=4, seed=5):
    """T = 32, F = 2: 32 live tracks, C = 32"""
    frames = []
    for f in range(2):
        frames.append([((0.1, -0.8 + 0.22 * (o % 8) + 0.01 * f, 0.1, -0.8 + 0.45 * (o // 8)), 0.9, float(o)) for o in range(32)])
    case = with_tracker(rows_from_objects(frames, 32, A, G, seed), 2, 1, iou_gate=0.05)
    assert case["num_tracks"].tolist() == [32]
    return case


def reference(case, horizon=0, **kw):
    return trajectory.reference_smooth(case["where"], case["n"], case["track_id"], case["num_tracks"], case["track_first"],
                                       case["track_last"], case["F"], case["max_age"], case["img"], horizon, what=case["what"],
                                       glimpse=case["glimpse"], score=case["score"], **kw)


# ---- the planted linear sequences: tx = a + f / 16, one sighting removed per track, max_age = 1, ground truth on the line ----------
PLANTED = dict(S=2, F=8, T=3, K=2, HZ=3, STEP=1.0 / 16, SCALE=0.3, TAU=0.5)


def planted_where(s, o, f):
    p = PLANTED
    return (p["SCALE"], -0.5 + 0.1 * o + 0.05 * s + f * p["STEP"], p["SCALE"], -0.5 + 1.0 * o)


def planted_sequences(A=5, G=16, seed=11):
    """(case, gt_boxes [S, F, K, 4], gt_future [S, HZ, K, 4], gaps): K objects per sequence on lines, each with ONE interior sighting
    removed; the ground truth is on the line in every frame, and goes on along it over the horizon"""
    p = PLANTED
    S, F, T, K = p["S"], p["F"], p["T"], p["K"]
    frames, gaps = [], 0
    for s in range(S):
        removed = {o: 2 + (3 * s + 2 * o) % (F - 3) for o in range(K)}         # an interior frame: 1 <= f <= F - 2
        gaps += K
        for f in range(F):
            frames.append([(planted_where(s, o, f), 0.9, float(o)) for o in range(K) if removed[o] != f])
    case = with_tracker(rows_from_objects(frames, T, A, G, seed), F, 1)
    assert case["num_tracks"].tolist() == [K] * S and (case["track_gaps"][:, :K] == 1).all()      # every track bridges its gap
    line = lambda frames_: np.array([[[planted_where(s, o, f) for o in range(K)] for f in frames_] for s in range(S)], np.float32)
    return case, scene_boxes(line(range(F)), IMG), scene_boxes(line(range(F, F + p["HZ"])), IMG), gaps


# ---- an independent smoother in matrix form ---------------------------------------------------------------------------------------------
def matrix_smoother(z, seen, q, r, vv):
    """z [n] float64, seen [n] bool (seen[0]): Kalman filter and RTS means with 2 x 2 matrices, numpy.linalg.inv.  Returns xs, vs [n]
    and the filtered (x, v) at the end"""
    A = np.array([[1.0, 1.0], [0.0, 1.0]])
    Q = q * np.array([[0.25, 0.5], [0.5, 1.0]])
    Hm = np.array([[1.0, 0.0]])
    m, P = np.array([z[0], 0.0]), np.diag([r, vv])
    filt, pred = [(m, P)], [None]
    for f in range(1, len(z)):
        mp, Pp = A @ m, A @ P @ A.T + Q
        pred.append((mp, Pp))
        if seen[f]:
            K = Pp @ Hm.T / (Pp[0, 0] + r)
            m, P = mp + (K * (z[f] - mp[0])).ravel(), Pp - K @ Hm @ Pp
        else:
            m, P = mp, Pp
        filt.append((m, P))
    ms = [None] * len(z)
    ms[-1] = filt[-1][0]
    for f in range(len(z) - 2, -1, -1):
        Cg = filt[f][1] @ A.T @ np.linalg.inv(pred[f + 1][1])
        ms[f] = filt[f][0] + Cg @ (ms[f + 1] - pred[f + 1][0])
    ms = np.array(ms)
    return ms[:, 0], ms[:, 1], filt[-1][0]
