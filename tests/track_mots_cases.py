"""Cases shared by test_track_mots_host.py and test_track_mots.py (numpy only): crafted cases of one mechanism each, built as tiny
owner / instance maps (4 x 8 pixels) or planted directly as a cont table, and a seeded generator whose owner map is a noisy copy of
the ground truth under a per-frame slot permutation, so that many mask IoUs fall around 1/2.  A case is dict(n [R], ids [T, R], T, G,
S, F) with either owner and gt [R, H, W] int8 (-1 = background) or cont [R, T+1, G+1] int32; `table(case)` gives the cont table of
either kind.  A crafted case carries `want`: the eight counters by name and `soft`."""
import numpy as np

H, W = 4, 8


def paint(*rects, shape=(H, W)):
    """a map of -1 with every (label, y0, y1, x0, x1) painted in order: rows y0..y1-1, columns x0..x1-1"""
    m = np.full(shape, -1, np.int8)
    for label, y0, y1, x0, x1 in rects:
        m[y0:y1, x0:x1] = label
    return m


def build(frames, T, G, want=None):
    """one sequence from frames = [(owner map, gt map, ids of the T steps, count), ...]"""
    F = len(frames)
    case = dict(owner=np.stack([f[0] for f in frames]), gt=np.stack([f[1] for f in frames]),
                ids=np.array([f[2] for f in frames], np.int32).reshape(F, T).T.copy(), n=np.array([f[3] for f in frames], np.int32),
                T=T, G=G, S=1, F=F)
    if want is not None:
        case["want"] = want
    return case


def table(case):
    """cont [R, T+1, G+1] int32 of a case: planted, or counted from its maps by plain loops (independent of track.mots_contingency)"""
    if "cont" in case:
        return case["cont"]
    T, G = case["T"], case["G"]
    owner, gt = case["owner"], case["gt"]
    cont = np.zeros((owner.shape[0], T + 1, G + 1), np.int32)
    for r in range(owner.shape[0]):
        for o, g in zip(owner[r].reshape(-1).tolist(), gt[r].reshape(-1).tolist()):
            if 0 <= o + 1 <= T and 0 <= g + 1 <= G:
                cont[r, o + 1, g + 1] += 1
    return cont


def stack(cases):
    """cases of one (T, G, F) as the sequences of one planted case"""
    T, G, F = cases[0]["T"], cases[0]["G"], cases[0]["F"]
    assert all((c["T"], c["G"], c["F"]) == (T, G, F) for c in cases)
    return dict(cont=np.concatenate([table(c) for c in cases]), n=np.concatenate([c["n"] for c in cases]),
                ids=np.concatenate([c["ids"] for c in cases], 1), T=T, G=G, S=sum(c["S"] for c in cases), F=F)


def counts(gt=0, tp=0, fn=0, fp=0, ids=0, mostly_tracked=0, mostly_lost=0, gt_objects=0, soft=0.0):
    return dict(gt=gt, tp=tp, fn=fn, fp=fp, ids=ids, mostly_tracked=mostly_tracked, mostly_lost=mostly_lost, gt_objects=gt_objects,
                soft=soft)


LEFT, RIGHT = (0, 4, 0, 3), (0, 4, 5, 8)                           # two masks of 12 pixels, two columns of background between them
BOTH = lambda a, b: paint((a,) + LEFT, (b,) + RIGHT)
ONE = lambda a: paint((a,) + LEFT)
WIDE = (0, 4, 0, 2)                                                # a ground-truth mask of 8 pixels

# two objects over 4 frames, every mask exact, each under one id; the steps change places in frame 2 (slots are not identities)
PERFECT = build([(BOTH(0, 1), BOTH(0, 1), [0, 1], 2), (BOTH(0, 1), BOTH(0, 1), [0, 1], 2), (BOTH(1, 0), BOTH(0, 1), [1, 0], 2),
                 (BOTH(0, 1), BOTH(0, 1), [0, 1], 2)], T=2, G=2,
                want=counts(gt=8, tp=8, mostly_tracked=2, gt_objects=2, soft=8.0))
# one object, id 0 and then id 1: tp 4, ids 1, MOTSA 3/4
SPLIT = build([(ONE(0), ONE(0), [0 if f < 2 else 1], 1) for f in range(4)], T=1, G=1,
              want=counts(gt=4, tp=4, ids=1, mostly_tracked=1, gt_objects=1, soft=4.0))
# the hypothesis holds exactly half of the ground-truth mask and nothing else: inter 4, union 8 -- no match: fn 1 and fp 1, MOTSA -1
EXACT_HALF = build([(paint((0, 0, 2, 0, 2)), paint((0,) + WIDE), [0], 1)], T=1, G=1,
                   want=counts(gt=1, fn=1, fp=1, mostly_lost=1, gt_objects=1))
# inter 5, union 8: a match, soft 0.625 exactly
FIVE_EIGHTHS = build([(paint((0, 0, 2, 0, 2), (0, 2, 3, 0, 1)), paint((0,) + WIDE), [0], 1)], T=1, G=1,
                     want=counts(gt=1, tp=1, mostly_tracked=1, gt_objects=1, soft=0.625))
# the object is unmatched for one frame and comes back under another id: the map persists, ids 1
GAP = build([(ONE(0), ONE(0), [0], 1), (ONE(-1), ONE(0), [0], 1), (ONE(0), ONE(0), [3], 1)], T=1, G=1,
            want=counts(gt=3, tp=2, fn=1, ids=1, gt_objects=1, soft=2.0))
# track_id -1 on a perfect mask: no hypothesis -- fn 1, fp 0
UNCONFIRMED = build([(ONE(0), ONE(0), [-1], 1)], T=1, G=1, want=counts(gt=1, fn=1, mostly_lost=1, gt_objects=1))
# step 1 has an id and not one pixel: counted nowhere
EMPTY_MASK = build([(ONE(0), ONE(0), [0, 5], 2)], T=2, G=1, want=counts(gt=1, tp=1, mostly_tracked=1, gt_objects=1, soft=1.0))
# two objects exchange their ids at mid-sequence: ids 2
SWAP = build([(BOTH(0, 1), BOTH(0, 1), [0, 1] if f < 2 else [1, 0], 2) for f in range(4)], T=2, G=2,
             want=counts(gt=8, tp=8, ids=2, mostly_tracked=2, gt_objects=2, soft=8.0))
# the slot is absent in frames 1 and 2 (frame 1 has a hypothesis on the background: fp) and returns under another id: ids 1
ABSENT_THEN_BACK = build([(ONE(0), ONE(0), [0], 1), (ONE(0), ONE(-1), [0], 1), (ONE(-1), ONE(-1), [0], 1), (ONE(0), ONE(0), [7], 1)],
                         T=1, G=1, want=counts(gt=2, tp=2, fp=1, ids=1, mostly_tracked=1, gt_objects=1, soft=2.0))
# nothing in any frame: every rate nan
NOTHING = build([(ONE(-1), ONE(-1), [-1], 0), (ONE(-1), ONE(-1), [-1], 0)], T=1, G=1, want=counts())
# planted: the row sum 2.6e9 passes int32 and 2 inter = 3.2e9 would too; inter 1.6e9 > union - inter = 1.1e9: soft = 1.6e9 / 2.7e9
BIG = dict(cont=np.array([[[0, 100000000], [1000000000, 1600000000]]], np.int32), n=np.array([1], np.int32),
           ids=np.array([[0]], np.int32), T=1, G=1, S=1, F=1,
           want=counts(gt=1, tp=1, mostly_tracked=1, gt_objects=1, soft=1.6e9 / 2.7e9))
# num_objects below 0 and above T: clipped to 0 (no hypothesis: fn) and to T (both steps are hypotheses)
CLIPPED = build([(BOTH(0, 1), BOTH(0, 1), [0, 1], -3), (BOTH(0, 1), BOTH(0, 1), [0, 1], 9), (BOTH(0, 1), BOTH(0, 1), [0, 1], 1)],
                T=2, G=2, want=counts(gt=6, tp=3, fn=3, gt_objects=2, soft=3.0))
CRAFTED = dict(PERFECT=PERFECT, SPLIT=SPLIT, EXACT_HALF=EXACT_HALF, FIVE_EIGHTHS=FIVE_EIGHTHS, GAP=GAP, UNCONFIRMED=UNCONFIRMED,
               EMPTY_MASK=EMPTY_MASK, SWAP=SWAP, ABSENT_THEN_BACK=ABSENT_THEN_BACK, NOTHING=NOTHING, BIG=BIG, CLIPPED=CLIPPED)


def mots_case(T, G, S, F, seed, shape=(4, 6)):
    """S sequences of F frames.  Ground truth: every pixel draws a label from -1..G-1, a slot is dropped from a frame now and then.
    Owner: the pixel's ground-truth slot sent through the frame's own permutation of slots to steps, replaced by a random label with a
    per-frame probability drawn from 0..0.7 -- so the mask IoUs spread around 1/2, exact halves included.  The step on slot g carries
    the id that follows g, which switches now and then and is -1 now and then; counts lie within -1..T+1."""
    rng = np.random.default_rng(seed)
    R = S * F
    owner, gt = np.full((R,) + shape, -1, np.int8), np.full((R,) + shape, -1, np.int8)
    ids, n = np.full((T, R), -1, np.int32), np.zeros(R, np.int32)
    for s in range(S):
        follows = rng.permutation(F * T + G)[:G]
        for f in range(F):
            r = s * F + f
            labels = rng.integers(-1, G, shape)
            for g in range(G):
                if rng.uniform() < 0.15:
                    labels[labels == g] = -1
            step_of = np.full(G + 1, -1)                           # slot -> step (index G: the background)
            steps = rng.permutation(T)
            step_of[:min(T, G)] = steps[:min(T, G)]
            own = step_of[labels]
            noisy = rng.uniform(size=shape) < rng.uniform(0.0, 0.7)
            own = np.where(noisy, rng.integers(-1, T, shape), own)
            gt[r], owner[r] = labels, own
            ids[:, r] = rng.integers(-1, F * T, T)
            for g in range(min(T, G)):
                if rng.uniform() < 0.15:
                    follows[g] = rng.integers(F * T + G)
                ids[step_of[g], r] = -1 if rng.uniform() < 0.1 else follows[g]
            n[r] = rng.integers(-1, T + 2)
    return dict(owner=owner, gt=gt, ids=ids, n=n, T=T, G=G, S=S, F=F)


def planted_case(T, G, S, F, seed, top=40):
    """a cont table planted directly: counts within 0..top, some frames with a dominant diagonal so that matches occur at every shape"""
    rng = np.random.default_rng(seed)
    R = S * F
    cont = rng.integers(0, top, (R, T + 1, G + 1)).astype(np.int32)
    for r in range(R):
        if rng.uniform() < 0.9:
            steps = rng.permutation(T)
            for g in range(min(T, G)):
                if rng.uniform() < 0.9:
                    cont[r, steps[g] + 1, g + 1] += rng.integers((T + G) * top // 4, 2 * (T + G) * top)    # around the row + column rest
        for g in range(G):
            if rng.uniform() < 0.15:
                cont[r, :, g + 1] = 0
        for j in range(T):
            if rng.uniform() < 0.1:
                cont[r, j + 1, :] = 0
    ids = rng.integers(-1, max(2, min(F * T, 6)), (T, R)).astype(np.int32)
    n = np.where(rng.uniform(size=R) < 0.3, rng.integers(-1, T + 2, R), T).astype(np.int32)      # mostly every step; some clipped
    return dict(cont=cont, n=n, ids=ids, T=T, G=G, S=S, F=F)
