"""Cases shared by test_track_optimal_host.py and test_track_optimal.py: the worked example, the chain, the planted ties of the
optimal association, crafted rows with their reference answer, and identity tables for air_track_idf."""
import numpy as np

from test_track_host import BOX, build_rows, crafted_rows

from attend_infer_repeat_amd import track

MARGIN = 1e-9
OBJ = lambda left: (BOX(left), 0.9, 0.0)

# w = 0, gate 0.1, boxes (left, 0, 10, 10): IoU for a shift d is (10 - d) / (10 + d).  Track A at left 10 (id 0), track B at left 18
# (id 1); object 0 at left 13 (A: 7/13, B: 1/3), object 1 at left 4 (A: 1/4, B: none).
WORKED = dict(frames=[[OBJ(10.0), OBJ(18.0)], [OBJ(13.0), OBJ(4.0)]], T=2, F=2, kw=dict(iou_gate=0.1, appearance_weight=0.0))
# gate 0.2.  Tracks at left 0, 6, 12 (ids 0, 1, 2); object 0 at left 2 (track 0: 8/12, track 1: 6/14), object 1 at left 8 (track 1:
# 8/12, track 2: 6/14; track 0: 2/18 is under the gate), object 2 at left -3 (track 0: 7/13 only).  Objects 0 and 1 go to tracks 0
# and 1 when they are inserted; object 2 re-routes both: an augmenting path over three tracks.
CHAIN = dict(frames=[[OBJ(0.0), OBJ(6.0), OBJ(12.0)], [OBJ(2.0), OBJ(8.0), OBJ(-3.0)]], T=3, F=2,
             kw=dict(iou_gate=0.2, appearance_weight=0.0))
# Exact ties.  ONE_TRACK: two objects at the same distance on either side of one track, profit P each: both assignments are worth P.
# Object 0 is inserted first and takes the track (u_0 = -P).  Object 1: the track's column has reduced cost -P, its own column 0, so
# the track's column enters the tree (u_1 = -P, its own column now at P), and with it object 0, whose own column (32 + 0) costs
# 0 - u_0 = P as well: of the two equal columns the lower one, object 0's, is the free column the path ends in -- object 0 gives the
# track up and is born, object 1 continues the track.  (The greedy rule keeps object 0 on the track: equal aff, the lower j.)
# TWO_TRACKS: two objects and two tracks, all four pairs alike: object 0 takes the lowest column (track 0); object 1 finds tracks 0
# and 1 at the same reduced cost, enters track 0's column first, and from object 0 track 1 costs no more than it did: it keeps the
# predecessor that gave it that cost first, the insertion itself -- object 1 takes track 1 and nothing moves.
TIE_ONE_TRACK = dict(frames=[[OBJ(10.0)], [OBJ(12.0), OBJ(8.0)]], T=2, F=2, kw=dict(iou_gate=0.1, appearance_weight=0.0))
TIE_TWO_TRACKS = dict(frames=[[OBJ(10.0), OBJ(14.0)], [OBJ(12.0), (BOX(12.0), 0.8, 0.0)]], T=2, F=2,
                      kw=dict(iou_gate=0.1, appearance_weight=0.0))


def planted(spec, matching="optimal"):
    """(case for the kernel, the reference's answer) of one of the planted specs above"""
    T, F = spec["T"], spec["F"]
    what, boxes, score, n = build_rows(spec["frames"], T)
    ref = track.reference_associate(what, boxes, score, n, F, matching=matching, **spec["kw"])
    return dict(what=what, boxes=boxes, score=score, n=n, T=T, A=2, S=len(spec["frames"]) // F, F=F, kw=spec["kw"]), ref


def crafted_optimal(T, A, S, F, seed, **kw):
    """test_track_host.crafted_rows (drifting objects, dropouts, clutter, non-finite entries, counts outside 0..T) with the answer of
    the optimal rule; every IoU at least MARGIN from the gate"""
    case, _ = crafted_rows(T, A, S, F, seed=seed, margin=MARGIN, **kw)
    ref = track.reference_associate(case["what"], case["boxes"], case["score"], case["n"], F, return_margins=True, matching="optimal",
                                    **kw)
    assert (ref["gate_margin"] >= MARGIN).all() and "round_margin" not in ref
    return case, ref


def full_table_rows(A=8, F=4, seed=0, spread=1.5):
    """T = 32 with all 32 slots live from frame 0 on: 32 boxes in a cluster whose spread decides how many pairs pass the gate
    (spread 1.5 with gate 0: every pair admissible; spread 40 with gate 0.3: sparse), jittered from frame to frame"""
    rng = np.random.default_rng(seed)
    T, R = 32, F
    centre = rng.uniform(0, spread, (T, 2))
    what, boxes, score = rng.normal(size=(T, R, A)).astype(np.float32), np.zeros((T, R, 4), np.float32), np.ones((T, R), np.float32)
    for f in range(F):
        order = rng.permutation(T)
        boxes[:, f, :2] = (centre + rng.normal(size=(T, 2)) * 0.3)[order]
        boxes[:, f, 2:] = 10.0 + rng.uniform(0, 1, (T, 2))
    return dict(what=what, boxes=boxes, score=score, n=np.full(R, T, np.int32), T=T, A=A, S=1, F=F)


def identity_case(T, S, F, G, seed, fresh_ids=False):
    """boxes, counts, track ids and ground truth for air_track_idf: G objects drift per sequence, hypotheses follow some of them
    under ids that switch now and then (fresh_ids: a new id in every frame), with clutter, duplicated ids inside a frame, ids of -1,
    non-finite boxes, absent ground-truth slots and counts outside 0..T"""
    rng = np.random.default_rng(seed)
    R = S * F
    boxes, ids = rng.uniform(0, 40, (T, R, 4)).astype(np.float32), np.full((T, R), -1, np.int32)
    n, gt = np.zeros(R, np.int32), np.zeros((R, G, 4), np.float32)
    for s in range(S):
        pos, vel = rng.uniform(5, 45, (G, 2)), rng.uniform(-1, 1, (G, 2))
        cur = rng.permutation(F * T)[:G]
        for f in range(F):
            r = s * F + f
            rows = []
            for g in range(G):
                box = np.array([pos[g, 0] + f * vel[g, 0], pos[g, 1] + f * vel[g, 1], 10.0, 10.0])
                if rng.uniform() < 0.85:
                    gt[r, g] = box
                if fresh_ids:
                    cur[g] = f * T + g % T
                elif rng.uniform() < 0.2:
                    cur[g] = rng.integers(F * T)
                if rng.uniform() < 0.8:
                    rows.append((box + rng.normal(size=4) * rng.choice([0.3, 2.0]), cur[g]))
            while rng.uniform() < 0.3:
                rows.append((rng.uniform(0, 40, 4), rng.integers(-1, F * T)))
            if rows and rng.uniform() < 0.3:                       # the same id twice in a frame
                rows.append((rows[0][0] + 0.2, rows[0][1]))
            rows = [rows[i] for i in rng.permutation(len(rows))][:T]
            for j, (box, i) in enumerate(rows):
                boxes[j, r], ids[j, r] = box, i
                if rng.uniform() < 0.03:
                    boxes[j, r, rng.integers(4)] = np.nan
            n[r] = len(rows) + (2 if len(rows) == T and rng.uniform() < 0.5 else 0)
    return dict(boxes=boxes, n=n, ids=ids, gt=gt, T=T, S=S, F=F, G=G)
