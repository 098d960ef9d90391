"""Cases shared by test_track_hota_host.py and test_track_hota.py (numpy only): seeded tables for air_track_hota -- G objects drift per
sequence, hypotheses follow some of them with jitter, drops, spurious boxes, id switches and splits -- and crafted cases with a
closed form or one mechanism each.  A case is dict(boxes [T, R, 4], n [R], ids [T, R], gt [R, G, 4], T, S, F, G) and, where the
table is narrower than F T, n_ids."""
import numpy as np

BOX = lambda left, top=0.0: [float(left), float(top), 10.0, 10.0]


def build(frames, T, G, n_ids=None):
    """one sequence from frames = [(hypotheses [(box, id), ...], ground truth [box or None, ...]), ...]"""
    F = len(frames)
    boxes, ids = np.zeros((T, F, 4), np.float32), np.full((T, F), -1, np.int32)
    n, gt = np.zeros(F, np.int32), np.zeros((F, G, 4), np.float32)
    for f, (hyps, gts) in enumerate(frames):
        n[f] = len(hyps)
        for j, (box, i) in enumerate(hyps):
            boxes[j, f], ids[j, f] = box, i
        for g, box in enumerate(gts):
            if box is not None:
                gt[f, g] = box
    case = dict(boxes=boxes, n=n, ids=ids, gt=gt, T=T, S=1, F=F, G=G)
    if n_ids is not None:
        case["n_ids"] = n_ids
    return case


def stack(cases):
    """cases of one (T, F, G) as the sequences of one case"""
    T, F, G = cases[0]["T"], cases[0]["F"], cases[0]["G"]
    assert all((c["T"], c["F"], c["G"]) == (T, F, G) for c in cases)
    return dict(boxes=np.concatenate([c["boxes"] for c in cases], 1), n=np.concatenate([c["n"] for c in cases]),
                ids=np.concatenate([c["ids"] for c in cases], 1), gt=np.concatenate([c["gt"] for c in cases]), T=T,
                S=sum(c["S"] for c in cases), F=F, G=G)


# every figure 1: two objects, each under one id, every box exact
PERFECT = build([([(BOX(2 * f), 0), (BOX(40 - f), 1)], [BOX(2 * f), BOX(40 - f)]) for f in range(4)], T=2, G=2)
# one object, id 0 in the first half and id 1 in the second: DetA 1, AssA 0.5
SPLIT = build([([(BOX(f), 0 if f < 2 else 1)], [BOX(f)]) for f in range(4)], T=1, G=1)
# one object found in the first half of its frames only: DetA = AssA = HOTA = 0.5
HALF_DETECTED = build([([(BOX(f), 0)] if f < 2 else [], [BOX(f)]) for f in range(4)], T=1, G=1)
# two objects far apart exchange their ids at mid-sequence
SWAP = build([([(BOX(f), 0 if f < 2 else 1), (BOX(40 + f), 1 if f < 2 else 0)], [BOX(f), BOX(40 + f)]) for f in range(4)], T=2, G=2)
# IoU exactly 0.25, 0.5 and 0.75: [0,0,4,1] on [0,0,1,1], [0,0,2,1] on [0,0,1,1], [0,0,4,1] on [0,0,3,1]
EXACT_LEVELS = build([([([0, 0, 4, 1], 0), ([10, 0, 2, 1], 1), ([20, 0, 4, 1], 2)], [[0, 0, 1, 1], [10, 0, 1, 1], [20, 0, 3, 1]])], T=3, G=3)
# id 0 follows the object at IoU 0.75 in all four frames; in frame 2 id 1 sits on it at IoU 1.  The potentials: frames 0, 1, 3 add 1
# to pot[0, 0]; frame 2 has rs = 1.75, so id 0 adds 0.75 / 1.75 and id 1 adds 1 / 1.75:  pot = 24/7 and 4/7, gc = 4, ic = 4 and 1,
# A = (24/7) / (8 - 24/7) = 0.75 and (4/7) / (5 - 4/7) = 4/31.  Frame 2: A sim = 0.5625 for id 0 against 0.129 for id 1 -- id 0 keeps the
# object although id 1 has the larger IoU.  tp = 4 up to alpha = 0.75 (15 thresholds), fp = 1; matches[a, 0, 0] = 4: AssA = 1 there.
DISTRACTOR = build([([([0, 0, 3, 1], 0)] + ([([0, 0, 4, 1], 1)] if f == 2 else []), [[0, 0, 4, 1]]) for f in range(4)], T=2, G=1)
# two hypotheses with one box and ids of identical histories: both assignments have the same profit
PROFIT_TIE = build([([(BOX(1), 0), (BOX(1), 1)], [BOX(0)]) for f in range(2)], T=2, G=1)
# id 0 twice in frame 0
DUPLICATE_ID = build([([(BOX(0), 0), (BOX(2), 0)], [BOX(0)]), ([(BOX(1), 0)], [BOX(1)]), ([(BOX(2), 0), (BOX(30), 1)], [BOX(2)])], T=2, G=1)
# ids 7 and 5 lie beyond a table of four ids
ID_BEYOND = build([([(BOX(f), 0), (BOX(f + 1), 7)], [BOX(f)]) for f in range(2)] + [([(BOX(2), 5)], [BOX(2)])], T=2, G=1, n_ids=4)
NONFINITE = build([([(BOX(0), 0), ([np.nan, 0, 10, 10], 1)], [BOX(0), BOX(30)]),
                   ([([1, 0, np.inf, 10], 0), (BOX(30), 1)], [BOX(1), BOX(30)]),
                   ([(BOX(2), 0), (BOX(30), 1)], [[np.nan, 0, 10, 10], BOX(30)]),
                   ([(BOX(3), 0), ([30, -np.inf, 10, 10], 1)], [BOX(3), [30, 0, np.nan, 10]])], T=2, G=2)
# a frame without a hypothesis, one without a present slot, one with neither, one with both
EMPTY_FRAMES = build([([], [BOX(0)]), ([(BOX(1), 0)], [None]), ([], [None]), ([(BOX(3), 0)], [BOX(3)])], T=1, G=1)
NOTHING = build([([], [None]), ([], [None])], T=1, G=1)
CRAFTED = dict(PERFECT=PERFECT, SPLIT=SPLIT, HALF_DETECTED=HALF_DETECTED, SWAP=SWAP, EXACT_LEVELS=EXACT_LEVELS, DISTRACTOR=DISTRACTOR,
               PROFIT_TIE=PROFIT_TIE, DUPLICATE_ID=DUPLICATE_ID, ID_BEYOND=ID_BEYOND, NONFINITE=NONFINITE, EMPTY_FRAMES=EMPTY_FRAMES,
               NOTHING=NOTHING)


def hota_case(T, S, F, G, seed, followers=1):
    """G objects drift per sequence; hypotheses follow some of them with jitter under ids that switch now and then (or split for
    good), with dropped detections, spurious boxes, an id twice in a frame, ids of -1, non-finite boxes, absent ground-truth slots
    and counts outside 0..T.  followers: the hypotheses on each object (4 with T = 32, G = 8: frames of 32 hypotheses)"""
    rng = np.random.default_rng(seed)
    R = S * F
    boxes, ids = rng.uniform(0, 40, (T, R, 4)).astype(np.float32), np.full((T, R), -1, np.int32)
    n, gt = np.zeros(R, np.int32), np.zeros((R, G, 4), np.float32)
    for s in range(S):
        pos, vel = rng.uniform(5, 45, (G, 2)), rng.uniform(-1, 1, (G, 2))
        cur = rng.permutation(F * T)[:G * followers].reshape(G, followers)
        for f in range(F):
            r = s * F + f
            rows = []
            for g in range(G):
                box = np.array([pos[g, 0] + f * vel[g, 0], pos[g, 1] + f * vel[g, 1], 10.0, 10.0])
                if rng.uniform() < 0.85:
                    gt[r, g] = box
                for q in range(followers):
                    if rng.uniform() < 0.15:
                        cur[g, q] = rng.integers(F * T)
                    if rng.uniform() < (0.8 if followers == 1 else 0.97):
                        rows.append((box + rng.normal(size=4) * rng.choice([0.3, 2.0]), cur[g, q]))
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


def trackeval_case(seed, F=10, G=3, T=5):
    """a clean table for the comparison with a TrackEval-style evaluation: G objects drift, each followed under one id with box
    jitter of 2 px and 20 % dropped detections, a spurious hypothesis now and then; every other seed splits one object's track into
    two ids at a random frame.  No id twice in a frame, no id of -1, nothing non-finite, every slot present."""
    rng = np.random.default_rng(seed)
    boxes, ids = np.zeros((T, F, 4), np.float32), np.full((T, F), -1, np.int32)
    n, gt = np.zeros(F, np.int32), np.zeros((F, G, 4), np.float32)
    pos, vel = rng.uniform(5, 45, (G, 2)), rng.uniform(-2, 2, (G, 2))
    split_g, split_f = (int(rng.integers(G)), int(rng.integers(1, F))) if seed % 2 else (-1, F)
    for f in range(F):
        rows = []
        for g in range(G):
            gt[f, g] = [pos[g, 0] + f * vel[g, 0], pos[g, 1] + f * vel[g, 1], 10.0, 10.0]
            if rng.uniform() < 0.8:
                rows.append((gt[f, g] + rng.normal(size=4) * 2.0, G + g if (g == split_g and f >= split_f) else g))
        if rng.uniform() < 0.3 and len(rows) < T:
            rows.append((rng.uniform(0, 40, 4), 2 * G + f))
        rows = [rows[i] for i in rng.permutation(len(rows))]
        for j, (box, i) in enumerate(rows):
            boxes[j, f], ids[j, f] = box, i
        n[f] = len(rows)
    return dict(boxes=boxes, n=n, ids=ids, gt=gt, T=T, S=1, F=F, G=G)
