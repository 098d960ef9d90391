"""Cases shared by test_track_stitch_host.py and test_track_stitch.py: planted provider rows (track_motion_cases.rows_from_where) whose
tracks a tracker with a small max_age splits, the tracker's reference output on them, seeded random batches, the 32-track and 33-track
cases, a greedy restatement of the linking step, and the planted defects of track.reference_stitch."""
import contextlib

import numpy as np

import track_motion_cases as MC

from attend_infer_repeat_amd import track

TRACK_KW = dict(MC.KW)                                             # iou_gate 0.1, appearance_weight 0: the tracker that splits the tracks
TABLES = ("track_first", "track_last", "track_length", "track_gaps")


def _obj(tx, seen, ty=lambda f: 0.0):
    """an object with 10 px boxes on the 50 px canvas, present in the frames `seen`"""
    return lambda f: (0.2, tx(f), 0.2, ty(f)) if f in seen else None


def _span(*ranges):
    return set(f for lo, hi in ranges for f in range(lo, hi + 1))


# one object at a constant rate (2.5 px a frame), gone for the 4 frames 4..7: max_age = 1 retires its track, it is born again as id 1
LONG_OCCLUSION = dict(objects=[_obj(lambda f: -0.6 + 0.1 * f, _span((0, 3), (8, 11)))], F=12, T=1, max_age=1,
                      tracker_ids=[[0]] * 4 + [[]] * 4 + [[1]] * 4, parent=[-1, 0], root=[0, 0], links=1,
                      first=[0, -1], last=[11, -1], length=[8, 0], gaps=[1, 0])
# A moves right and B left; both are gone in the frames 4..6 and have passed each other when they come back in frame 7, each a little
# off its prediction (A 0.07 -> 0.11, B 0.00 -> 0.05): the pair of the largest affinity is (A, B's reappearance), and once greedy has
# taken it B is left with A's reappearance, far off.  The optimal assignment keeps A with A and B with B.
TWO_BEHIND = dict(objects=[_obj(lambda f: -0.63 + 0.1 * f if f < 7 else 0.11 + 0.1 * (f - 7), _span((0, 3), (7, 9))),
                           _obj(lambda f: 0.70 - 0.1 * f if f < 7 else 0.05 - 0.1 * (f - 7), _span((0, 3), (7, 9)))], F=10, T=2,
                  max_age=1, tracker_ids=[[0, 1]] * 4 + [[]] * 3 + [[2, 3]] * 3, parent=[-1, -1, 0, 1], root=[0, 1, 0, 1], links=2,
                  first=[0, 0, -1, -1], last=[9, 9, -1, -1], length=[7, 7, 0, 0], gaps=[1, 1, 0, 0], greedy_parent=[-1, -1, 1, 0])
# one object gone twice (3..5 and 9..11): three fragments, the links 0 -> 1 -> 2
CHAIN = dict(objects=[_obj(lambda f: -0.7 + 0.1 * f, _span((0, 2), (6, 8), (12, 13)))], F=14, T=1, max_age=1,
             tracker_ids=[[0]] * 3 + [[]] * 3 + [[1]] * 3 + [[]] * 3 + [[2]] * 2, parent=[-1, 0, 1], root=[0, 0, 0], links=2,
             first=[0, -1, -1], last=[13, -1, -1], length=[8, 0, 0], gaps=[2, 0, 0])
# LONG_OCCLUSION's rows under max_gap = 4: the gap is 5 = max_gap + 1
TOO_LATE = dict(LONG_OCCLUSION, stitch=dict(max_gap=4), parent=[-1, -1], root=[0, 1], links=0, first=[0, 8], last=[3, 11],
                length=[4, 4], gaps=[0, 0])
# the object comes back 12.5 px off its line: beyond the gate
TOO_FAR = dict(objects=[_obj(lambda f: -0.6 + 0.1 * f, _span((0, 3), (8, 11)), ty=lambda f: 0.5 if f >= 8 else 0.0)], F=12, T=1, max_age=1,
               tracker_ids=[[0]] * 4 + [[]] * 4 + [[1]] * 4, parent=[-1, -1], root=[0, 1], links=0, first=[0, 8], last=[3, 11],
               length=[4, 4], gaps=[0, 0])
# a static object ends; two begin later, mirrored about its line (ty = -0.1 and +0.1: e3 = -+0.1 exactly, so equal d2 bit for bit); the
# second carries the ended track's `what` code, the first another: with w = 0.5 the `what` rows decide
LOOKALIKE = dict(objects=[_obj(lambda f: 0.0, _span((0, 3))), _obj(lambda f: 0.0, _span((7, 9)), ty=lambda f: -0.1),
                          _obj(lambda f: 0.0, _span((7, 9)), ty=lambda f: 0.1)], F=10, T=2, max_age=1,
                 what={0: (1.0, 0.0), 1: (0.0, 1.0), 2: (1.0, 0.0)}, stitch=dict(appearance_weight=0.5),
                 tracker_ids=[[0]] * 4 + [[]] * 3 + [[1, 2]] * 3, parent=[-1, -1, 0], root=[0, 1, 0], links=1,
                 first=[0, 7, -1], last=[9, 9, -1], length=[7, 3, 0], gaps=[1, 0, 0])
SCENARIOS = dict(LONG_OCCLUSION=LONG_OCCLUSION, TWO_BEHIND=TWO_BEHIND, CHAIN=CHAIN, TOO_LATE=TOO_LATE, TOO_FAR=TOO_FAR,
                 LOOKALIKE=LOOKALIKE)


def scenario(spec, S=1, A=2):
    """the provider rows of a scenario (S identical sequences), its `what` codes planted per object"""
    case = MC.rows_from_where(spec["objects"], spec["F"], spec["T"], A=A, S=S)
    for g, code in spec.get("what", {}).items():
        for r in range(S * spec["F"]):
            if spec["objects"][g](r % spec["F"]) is None:
                continue
            j = sum(1 for o in spec["objects"][:g] if o(r % spec["F"]) is not None)
            case["what"][j, r, :len(code)] = code
    case["max_age"] = spec["max_age"]
    return case


def tracked(case, motion=None, **kw):
    """the reference tracker on the rows of a case: last-box association, or with motion = a dict of noise terms ({}: the defaults)"""
    rule = dict(TRACK_KW, max_age=case.get("max_age", 1), **kw)
    if motion is None:
        return MC.associate_last_box(case, **rule)
    return MC.associate_motion(case, return_state=True, **dict(rule, **motion))


def stitch(case, out, **kw):
    """track.reference_stitch on a case and the tracker's output on it"""
    return track.reference_stitch(case["what"], case["where"], out["track_id"], out["num_tracks"], out["track_first"], out["track_last"],
                                  out["track_length"], out["track_gaps"], case["F"], **kw)


def random_case(T, A, S, F, seed, max_age=0, motion=False, matching="greedy"):
    """MC.random_case's rows (objects at a constant rate with jitter, dropouts longer than max_age, clutter, planted NaN / inf in what,
    where, boxes and score) and the reference tracker's output on them: with motion the tracker's own, else the last-box tracker's --
    whose tracks may hold sightings with a non-finite `where` value"""
    case, ref = MC.random_case(T, A, S, F, seed, max_age=max_age, matching=matching, drop=0.3)
    case["max_age"] = max_age
    if not motion:
        ref = MC.associate_last_box(case, max_age=max_age, matching=matching)
    return case, ref


# (T, A, S, F, seed, max_age, motion): T <= 4, F <= 12, S <= 4, A in {2, 8, 50}
RANDOM = [(4, 2, 4, 12, 1, 0, False), (3, 8, 3, 12, 2, 1, True), (4, 50, 2, 11, 3, 0, True), (2, 8, 4, 9, 4, 0, False)]
RANDOM_STITCH = dict(max_gap=3, appearance_weight=0.25)


def full_case(n_before=16, n_after=16, A=8):
    """T = 32, F = 4: n_before objects in frame 0, none in frames 1 and 2, n_after of them back in frame 3, drifted: with max_age = 1
    that is n_before + n_after tracks -- 32 (every row and every slot column of the solver in use) or, with 17 + 16, one too many"""
    T, F = 32, 4
    place = lambda g: (-0.875 + 0.25 * (g % 8), -0.6 + 0.4 * (g // 8))
    objects = [(lambda f, g=g: (0.1, place(g)[0] + 0.01 * f, 0.1, place(g)[1] + 0.004 * f * (1 + g % 3))
                if f == 0 or (f == 3 and g < n_after) else None) for g in range(n_before)]
    case = MC.rows_from_where(objects, F, T, A=A)
    codes = np.random.default_rng(7).normal(size=(n_before, A)).astype(np.float32)
    for f in (0, 3):
        for j in range(int(case["n"][f])):
            case["what"][j, f] = codes[j]
    case["max_age"] = 1
    return case


def inconsistent_case(seed, T=2, A=8, S=6, F=9):
    """rows with tables no tracker would write: first / last frames outside 0 .. F - 1 and in either order, num_tracks from -1 to 40
    (above F T = 18 and above 32), ids in track_id up to 35 and twice in a frame, lengths and gaps at random -- what the rule's clips
    are for (STITCHING: the frames and N are clipped before use)"""
    rng = np.random.default_rng(seed)
    case, _ = MC.random_case(T, A, S, F, seed, max_age=0, drop=0.3)
    R, FT = S * F, F * T
    tracks = dict(track_id=rng.integers(-1, 8, (T, R)).astype(np.int32), num_tracks=rng.integers(-1, 41, S).astype(np.int32),
                  track_first=rng.integers(-3, F + 3, (S, FT)).astype(np.int32), track_last=rng.integers(-3, F + 3, (S, FT)).astype(np.int32),
                  track_length=rng.integers(0, 9, (S, FT)).astype(np.int32), track_gaps=rng.integers(0, 4, (S, FT)).astype(np.int32))
    tracks["track_id"][rng.uniform(size=(T, R)) < 0.1] = 35
    tracks["num_tracks"][:3] = (40, 25, 7)                         # OVERFLOW, clipped to F T, and as it is
    return case, tracks


def greedy_parent(pairs, s, n):
    """the linking step restated greedily: the admissible pair of the largest affinity first (equal: the lower a, then the lower b),
    its a and its b then closed"""
    open_pairs = {(a, b): v[2] for (q, a, b), v in pairs.items() if q == s and v[2] is not None}
    parent = [-1] * n
    while open_pairs:
        a, b = min(open_pairs, key=lambda ab: (-open_pairs[ab], ab[0], ab[1]))
        parent[b] = a
        open_pairs = {ab: v for ab, v in open_pairs.items() if ab[0] != a and ab[1] != b}
    return parent


# ---- the planted defects of the reference --------------------------------------------------------------------------------------------------
DEFECTS = ("gv_for_the_prediction", "first_sighting_of_a", "strict_gate", "gaps_without_the_link")


@contextlib.contextmanager
def planted(defect):
    """track.reference_stitch with one statement of the rule replaced (None: the rule itself)"""
    saved = {k: getattr(track, k) for k in ("_motion_predicted_state", "_stitch_ends", "_gated_pair", "_stitch_gaps")}

    def gv(filt, m, q, r):                                         # the mean in one product; the covariance as the rule has it
        xp, s = saved["_motion_predicted_state"](filt, m, q, r)
        return filt[0] + np.float64(m) * filt[1], s

    def strict(d2, msd, w, gate, pred_box, box):
        return None if not d2 < gate else saved["_gated_pair"](d2, msd, w, gate, pred_box, box)

    bad = {"gv_for_the_prediction": ("_motion_predicted_state", gv),
           "first_sighting_of_a": ("_stitch_ends", lambda sa, sb: (sa[0], sb[0])),
           "strict_gate": ("_gated_pair", strict),
           "gaps_without_the_link": ("_stitch_gaps", lambda gaps, links: gaps)}
    if defect is not None:
        setattr(track, *bad[defect])
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(track, k, v)
