"""Cases shared by tests/test_temporal_host.py (float64 only) and tests/test_temporal.py (the same cases on the device): random rows for
air_temporal_pool with neighbours that overlap, repeat and tie, and the planted sequence -- one sequence of three frames whose middle
frame's parse misses an object both neighbours hold."""
import numpy as np

from attend_infer_repeat_amd import prune, temporal

OUT_TOL, OUT_L2 = 1e-4, 3e-5                                       # test_engine.py's bars for per-sample outputs (the GPU tests assert so)
MULT, STD = 0.5, 0.3                                               # test_prune.py's
PRIORS = (0.0, 1.0, 0.3, 0.5, 0.0, 1.0)                            # test_propose.py's: what, where scale, where shift (loc, scale)


def chain(n, T):
    return (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(np.float32)


def pool_rows(T, S, F, A, G, seed):
    """current rows of R = S F frames whose objects sit at a few shared places, so that every state occurs: a neighbour's object at a
    current object's place (KNOWN), at a free place (TAKEN / FULL), twice at one free place (DUPLICATE, partners), equal scores (the
    lower q), a NaN and an inf among the values (NONFINITE), and counts from 0 to T and beyond (clipped)."""
    rng = np.random.default_rng(seed)
    R = S * F
    places = np.array([(-0.6, -0.6), (0.6, 0.6), (0.6, -0.6), (-0.6, 0.6), (0.0, 0.0), (0.0, 0.6), (0.0, -0.6)])
    where = np.empty((T, R, 4), np.float32)
    where[..., 0::2] = rng.uniform(0.25, 0.35, (T, R, 2))
    pick = rng.integers(0, len(places), (T, R))
    where[..., 1], where[..., 3] = places[pick, 0], places[pick, 1]
    where[..., 1::2] += rng.normal(size=(T, R, 2)).astype(np.float32) * 0.03      # near, not at: IoUs on both sides of the bar
    score = rng.choice([0.2, 0.5, 0.5, 0.8, 0.9], (T, R)).astype(np.float32)      # ties are common
    what = rng.normal(size=(T, R, A)).astype(np.float32)
    glimpse = rng.normal(size=(T, R, G)).astype(np.float32)
    n = rng.integers(0, T + 1, R)
    n[0] = T
    if R > 1:
        n[1] = T + 3                                               # clipped to T
    if R > 2:
        n[2] = 0
    if R > 3:
        n[R - 1] = T
        what[0, R - 1, A - 1] = np.nan                             # a candidate of frame R - 2 (when that is the same sequence)
        where[T - 1, 0, 2] = np.inf
        score[T - 1, 1] = np.nan
    return dict(what=what, where=where, glimpse=glimpse, score=score, n=n, prior=rng.uniform(0.1, 1.0, T + 1))


# ---- the planted sequence -----------------------------------------------------------------------------------------------------------------
PLANTED = dict(S=1, F=3, T=2, P=1, A=4, img=(16, 16), crop=(4, 4))
PLACE_A = (0.3, -0.5, 0.3, -0.5)                                   # where = [sx, tx, sy, ty]: the object every frame's parse holds
PLACE_B = (0.3, 0.4, 0.3, 0.3)                                     # the second object's place in frame 1
STEP_B = (0.0, 0.05, 0.0, 0.05)                                    # its motion per frame: 0.4 pixels each way on the 16 x 16 canvas


def planted_sequence(motion=True):
    """Frames 0 and 2 hold both objects (n = 2), frame 1's rows only the first (n = 1; its slot 1 is a stale row far from everything);
    all three observations show both.  The second object moves by STEP_B per frame (motion=False: it stands still), so its `where` rows
    in frames 0 and 2 are symmetric about its frame-1 place.  Returns the rows as air_temporal_pool takes them, obs [3, 16, 16] fp32,
    and `truth`: the second object's where row per frame."""
    rng = np.random.default_rng(5)
    T, R, A = PLANTED["T"], PLANTED["F"], PLANTED["A"]
    h, w = PLANTED["crop"]
    g = rng.uniform(0.5, 1.0, (2, h, w)).astype(np.float32)        # the two objects' glimpses: the same in every frame
    z = (rng.normal(size=(2, A)) * 0.3).astype(np.float32)
    step = np.array(STEP_B if motion else (0.0,) * 4, np.float32)
    truth = np.stack([np.array(PLACE_B, np.float32) + (f - 1) * step for f in range(R)], 0)
    where = np.empty((T, R, 4), np.float32)
    where[0], where[1] = np.array(PLACE_A, np.float32), truth
    where[1, 1] = (0.2, -0.1, 0.2, 0.8)                            # frame 1, slot 1: absent (n = 1)
    glimpse = np.stack([np.broadcast_to(g[0].reshape(-1), (R, h * w)), np.broadcast_to(g[1].reshape(-1), (R, h * w))], 0).copy()
    what = np.stack([np.broadcast_to(z[0], (R, A)), np.broadcast_to(z[1], (R, A))], 0).copy()
    score = np.array([[0.9, 0.9, 0.9], [0.8, 0.1, 0.7]], np.float32)        # the frame-0 sighting of the second object ranks first
    n = np.array([2, 1, 2])
    layers = [prune._st_write(np.broadcast_to(g[k].astype(np.float64), (R, h, w)),
                              (np.broadcast_to(np.array(PLACE_A, np.float64), (R, 4)) if k == 0 else truth.astype(np.float64)),
                              PLANTED["img"]) for k in range(2)]
    obs = (MULT * (layers[0] + layers[1])).astype(np.float32)
    return dict(what=what, where=where, glimpse=glimpse, score=score, n=n, prior=np.array([0.2, 0.3, 0.5]), obs=obs, truth=truth)


def planted_reference(case, interpolate, both_sides=True, iou_novel=0.3):
    """reference_pool -> prune.reference_score -> prune.reference_select (T := C) -> the provenance, all in float64"""
    from attend_infer_repeat_amd import propose
    T, P = PLANTED["T"], PLANTED["P"]
    h, w = PLANTED["crop"]
    pool = temporal.reference_pool(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["prior"], PLANTED["F"],
                                   PLANTED["img"], P, iou_novel, both_sides, interpolate)
    C, R = T + P, PLANTED["F"]
    rec = prune.reference_score(pool["glimpse"].reshape(C, R, h, w), pool["where"], pool["presence"], case["obs"], MULT, STD, 1)
    sel = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, PRIORS,
                                 pool["prior"], 1, 1, rec)
    sel["source_out"] = propose.reference_source(pool["source"], sel["kept_step"])
    return pool, rec, sel
