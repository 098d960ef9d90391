"""Host-side tests of sequence tracking (attend_infer_repeat_amd/track.py, data.create_moving_mnist): `reference_associate` and
`reference_score` against answers written out by hand, the argument checks, the moving-digit generator.  No GPU.

One case departs from how the issue words it.  The issue's OVERFLOW case (T = 32, max_age = 1: 32 objects, then 32 others far away)
expects the slots free in frame 2; by the issue's own rule (births come before ageing, a track is retired when age > max_age) the 32
coasting tracks are still live when frame 2's births are decided -- they may yet be matched in frame 2, which is what "an object
missing for max_age frames comes back under its id" needs -- so frame 2 overflows as well and frame 3 has the slots free.  The test
states that, and shows frame 2 free with max_age = 0."""
import numpy as np
import pytest

from attend_infer_repeat_amd import track
from attend_infer_repeat_amd.data import _bounce, _tight_box, create_moving_mnist, procedural_moving_mnist
from attend_infer_repeat_amd.tile import box_iou


# ---- helpers shared with test_track.py ------------------------------------------------------------------------------------------------
def build_rows(frames, T, A=2):
    """provider rows from a list, per row r = s * F + f, of objects (box (l, t, w, h), score, what: a number or A numbers): what
    [T, R, A], boxes [T, R, 4], score [T, R] fp32 and num_objects [R] int32"""
    R = len(frames)
    what, boxes, score = np.zeros((T, R, A), np.float32), np.zeros((T, R, 4), np.float32), np.zeros((T, R), np.float32)
    n = np.zeros(R, np.int32)
    for r, objs in enumerate(frames):
        assert len(objs) <= T
        for j, (box, sc, wh) in enumerate(objs):
            boxes[j, r], score[j, r], what[j, r] = box, sc, wh
        n[r] = len(objs)
    return what, boxes, score, n


def crafted_rows(T, A, S, F, seed, margin=1e-9, **kw):
    """random provider rows around a few true objects per sequence that drift with jitter, with dropouts, clutter, low scores,
    non-finite entries, a shuffled slot order per frame and counts outside 0..T; redrawn until every IoU is at least `margin` from the
    gate and every greedy round's winner beats the runner-up by at least `margin`.  Returns the rows and the reference's answer."""
    R = S * F
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        what, boxes, score = (rng.normal(size=(T, R, A)).astype(np.float32), rng.uniform(0, 40, (T, R, 4)).astype(np.float32),
                              rng.uniform(size=(T, R)).astype(np.float32))
        n = np.zeros(R, np.int32)
        for s in range(S):
            k = int(rng.integers(1, min(T, 12) + 1))
            pos, vel = rng.uniform(5, 45, (k, 2)), rng.uniform(-2, 2, (k, 2))
            size, code = rng.uniform(6, 14, (k, 2)), rng.normal(size=(k, A))
            for f in range(F):
                r, objs = s * F + f, []
                for o in range(k):
                    if rng.uniform() < 0.8:                        # (else: a dropout)
                        c, wh = pos[o] + f * vel[o] + rng.normal(size=2) * 0.3, size[o] + rng.normal(size=2) * 0.2
                        objs.append((c[0] - wh[0] / 2, c[1] - wh[1] / 2, wh[0], wh[1], rng.uniform(0.3, 1.0),
                                     code[o] + rng.normal(size=A) * 0.05))
                while rng.uniform() < 0.3:                         # clutter
                    objs.append((rng.uniform(0, 40), rng.uniform(0, 40), rng.uniform(4, 12), rng.uniform(4, 12), rng.uniform(),
                                 rng.normal(size=A)))
                objs = [objs[i] for i in rng.permutation(len(objs))][:T]
                for j, o in enumerate(objs):
                    boxes[j, r], score[j, r], what[j, r] = o[:4], o[4], o[5]
                    u = rng.uniform()
                    if u < 0.02:
                        boxes[j, r, rng.integers(4)] = rng.choice([np.nan, np.inf, -np.inf])
                    elif u < 0.04:
                        score[j, r] = rng.choice([np.nan, np.inf])
                    elif u < 0.06:
                        what[j, r, rng.integers(A)] = rng.choice([np.nan, -np.inf])
                n[r] = len(objs)
                if len(objs) == T and rng.uniform() < 0.5:
                    n[r] = T + 2                                   # clipped to T
                elif rng.uniform() < 0.03:
                    n[r] = -1                                      # clipped to 0
        ref = track.reference_associate(what, boxes, score, n, F, return_margins=True, **kw)
        if (ref["gate_margin"] >= margin).all() and (ref["round_margin"] >= margin).all():
            return dict(what=what, boxes=boxes, score=score, n=n, T=T, A=A, S=S, F=F, kw=kw), ref
    raise AssertionError("no crafted case within the margins")


def moving_gt(case, rng, G):
    """ground truth for a crafted case: per sequence G slots that follow some of the tracked boxes loosely, with absent rows"""
    T, S, F = case["T"], case["S"], case["F"]
    gt = np.zeros((S * F, G, 4), np.float32)
    for r in range(S * F):
        n = int(np.clip(case["n"][r], 0, T))
        for g in range(G):
            if n and rng.uniform() < 0.7:
                j = int(rng.integers(n))
                if np.isfinite(case["boxes"][j, r]).all():
                    gt[r, g] = case["boxes"][j, r] + rng.normal(size=4).astype(np.float32) * 0.5
    return gt


BOX = lambda x, y=0.0: (x, y, 10.0, 10.0)
OUTPUTS = ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot", "num_tracks", "track_first", "track_last", "track_length",
           "track_gaps", "state_counts")


def associate(frames, T, F, A=2, **kw):
    what, boxes, score, n = build_rows(frames, T, A)
    return track.reference_associate(what, boxes, score, n, F, **kw)


# ---- reference_associate --------------------------------------------------------------------------------------------------------------
CROSSING = [[(BOX(0.0), 0.9, 0.0), (BOX(12.0), 0.9, 5.0)], [(BOX(8.0), 0.9, 0.0), (BOX(4.0), 0.9, 5.0)]]


def test_crossing_objects_swap_ids_on_iou_alone_and_keep_them_with_appearance():
    iou_stay, iou_swap = box_iou(BOX(0.0), BOX(8.0)), box_iou(BOX(0.0), BOX(4.0))
    assert iou_stay == 20.0 / 180.0 and iou_swap == 60.0 / 140.0 and iou_stay > 0.1
    for w, swapped in ((0.0, True), (0.5, False)):
        stay, swap = (1 - w) * iou_stay + w / (1 + 0.0), (1 - w) * iou_swap + w / (1 + 25.0)
        assert (swap - stay if swapped else stay - swap) >= 1e-6   # the gap that decides, on both tracks alike (the case is symmetric)
        out = associate(CROSSING, 2, 2, iou_gate=0.1, appearance_weight=w)
        assert out["track_id"][:, 0].tolist() == [0, 1]
        assert out["track_id"][:, 1].tolist() == ([1, 0] if swapped else [0, 1])
        assert out["obj_state"][:, 1].tolist() == [track.MATCHED] * 2 and out["prev_frame"][:, 1].tolist() == [0, 0]
        assert out["prev_slot"][:, 1].tolist() == ([1, 0] if swapped else [0, 1])
        assert out["affinity"][0, 1] == np.float32(swap if swapped else stay)
        assert out["num_tracks"].tolist() == [2] and out["track_length"][0, :2].tolist() == [2, 2]


def test_an_object_missing_for_max_age_frames_comes_back_under_its_id():
    out = associate([[(BOX(0.0), 0.9, 1.0)], [], [(BOX(1.0), 0.9, 1.0)]], 2, 3, max_age=1)
    assert out["track_id"][0].tolist() == [0, -1, 0] and out["obj_state"][0].tolist() == [track.BORN, track.ABSENT, track.MATCHED]
    assert out["prev_frame"][0, 2] == 0 and out["prev_slot"][0, 2] == 0                      # (the sighting before the gap)
    assert out["num_tracks"].tolist() == [1]
    assert (out["track_first"][0, 0], out["track_last"][0, 0], out["track_length"][0, 0], out["track_gaps"][0, 0]) == (0, 2, 2, 1)
    assert out["track_first"][0, 1:].tolist() == [-1] * 5 and out["track_length"][0, 1:].tolist() == [0] * 5


def test_an_object_missing_for_max_age_plus_one_frames_gets_a_new_id():
    out = associate([[(BOX(0.0), 0.9, 1.0)], [], [], [(BOX(0.0), 0.9, 1.0)]], 1, 4, max_age=1)
    assert out["track_id"][0].tolist() == [0, -1, -1, 1] and out["obj_state"][0, 3] == track.BORN
    assert out["num_tracks"].tolist() == [2] and out["track_last"][0, :2].tolist() == [0, 3]
    assert out["track_gaps"][0, :2].tolist() == [0, 0] and out["track_length"][0, :2].tolist() == [1, 1]
    # and two frames are bridged with max_age = 2
    out = associate([[(BOX(0.0), 0.9, 1.0)], [], [], [(BOX(0.0), 0.9, 1.0)]], 1, 4, max_age=2)
    assert out["track_id"][0].tolist() == [0, -1, -1, 0] and out["track_gaps"][0, 0] == 1 and out["prev_frame"][0, 3] == 0


def test_an_object_below_birth_score_is_unconfirmed_yet_continues_a_track():
    out = associate([[(BOX(0.0), 0.9, 1.0)], [(BOX(1.0), 0.2, 1.0), (BOX(30.0), 0.2, 1.0)]], 2, 2, birth_score=0.5)
    assert out["obj_state"][:, 1].tolist() == [track.MATCHED, track.UNCONFIRMED] and out["track_id"][:, 1].tolist() == [0, -1]
    assert out["affinity"][1, 1] == 0 and out["prev_frame"][1, 1] == -1
    # exactly at the bar is born
    out = associate([[(BOX(0.0), 0.5, 1.0)]], 1, 1, birth_score=0.5)
    assert out["obj_state"][0, 0] == track.BORN


def _overflow_frames(F):
    return [[((20.0 * i, 1000.0 * f, 10.0, 10.0), 0.9, float(i)) for i in range(32)] for f in range(F)]


def test_overflow_while_coasting_tracks_hold_every_slot():
    out = associate(_overflow_frames(4), 32, 4, max_age=1)
    state = out["obj_state"]
    assert (state[:, 0] == track.BORN).all() and out["track_id"][:, 0].tolist() == list(range(32))
    assert (state[:, 1] == track.OVERFLOW).all() and (out["track_id"][:, 1] == -1).all()
    assert (state[:, 2] == track.OVERFLOW).all()                   # the coasting tracks could still be matched in frame 2: not free yet
    assert (state[:, 3] == track.BORN).all() and out["track_id"][:, 3].tolist() == list(range(32, 64))
    assert out["num_tracks"].tolist() == [64] and out["state_counts"][0].tolist() == [0, 0, 64, 0, 64, 0]
    assert (out["track_last"][0, :32] == 0).all() and (out["track_first"][0, 32:64] == 3).all() and (out["track_first"][0, 64:] == -1).all()
    out = associate(_overflow_frames(3), 32, 3, max_age=0)         # nothing coasts: the slots are free in frame 2
    assert (out["obj_state"][:, 1] == track.OVERFLOW).all() and (out["obj_state"][:, 2] == track.BORN).all()
    assert out["track_id"][:, 2].tolist() == list(range(32, 64))


@pytest.mark.parametrize("bad", ["box", "score", "what"])
def test_a_nonfinite_object_neither_matches_nor_is_born(bad):
    what, boxes, score, n = build_rows([[(BOX(0.0), 0.9, 1.0)], [(BOX(0.0), 0.9, 1.0), (BOX(30.0), 0.9, 1.0)]], 2)
    if bad == "box":
        boxes[0, 1, 2] = np.nan
    elif bad == "score":
        score[0, 1] = np.nan
    else:
        what[0, 1, 1] = np.inf
    out = track.reference_associate(what, boxes, score, n, 2)
    assert out["obj_state"][:, 1].tolist() == [track.NONFINITE, track.BORN] and out["track_id"][:, 1].tolist() == [-1, 1]
    assert out["state_counts"][0].tolist() == [1, 0, 2, 0, 0, 1] and out["track_length"][0, 0] == 1


TIE_ONE_TRACK = [[(BOX(0.0), 0.9, 1.0)], [(BOX(2.0), 0.9, 1.0), (BOX(-2.0), 0.9, 1.0)]]
TIE_TWO_TRACKS = [[(BOX(2.0), 0.9, 1.0), (BOX(-2.0), 0.9, 1.0)], [(BOX(0.0), 0.9, 1.0)]]


def test_a_planted_exact_tie_goes_to_the_lower_track_id_then_the_lower_slot():
    assert box_iou(BOX(0.0), BOX(2.0)) == box_iou(BOX(0.0), BOX(-2.0)) > 0.1
    out = associate(TIE_ONE_TRACK, 2, 2)                           # one track, two objects with equal aff: the lower j
    assert out["track_id"][:, 1].tolist() == [0, 1] and out["obj_state"][:, 1].tolist() == [track.MATCHED, track.BORN]
    out = associate([TIE_ONE_TRACK[0], TIE_ONE_TRACK[1][::-1]], 2, 2)
    assert out["track_id"][:, 1].tolist() == [0, 1]                # (still slot 0, now the other box)
    out = associate(TIE_TWO_TRACKS, 2, 2)                          # two tracks, one object with equal aff: the lower id
    assert out["track_id"][0, 1] == 0 and out["prev_slot"][0, 1] == 0 and out["track_length"][0, :2].tolist() == [2, 1]
    out = associate([TIE_TWO_TRACKS[0][::-1], TIE_TWO_TRACKS[1]], 2, 2)
    assert out["track_id"][0, 1] == 0 and out["prev_slot"][0, 1] == 0
    ref = associate(TIE_ONE_TRACK, 2, 2, return_margins=True)
    assert ref["round_margin"][0] == 0.0


def test_one_frame_gives_ids_in_slot_order():
    out = associate([[(BOX(30.0), 0.9, 1.0), (BOX(0.0), 0.8, 1.0), (BOX(15.0), 0.7, 1.0)]], 4, 1)
    assert out["track_id"][:, 0].tolist() == [0, 1, 2, -1] and out["num_tracks"].tolist() == [3]
    assert out["obj_state"][:, 0].tolist() == [track.BORN] * 3 + [track.ABSENT]
    assert out["track_first"][0].tolist() == [0, 0, 0, -1] and out["track_last"][0].tolist() == [0, 0, 0, -1]


@pytest.mark.parametrize("T,A,S,F", [(3, 5, 3, 5), (6, 1, 2, 17), (32, 3, 1, 4)])
def test_state_counts_sum_to_the_objects_of_a_sequence(T, A, S, F):
    case, ref = crafted_rows(T, A, S, F, seed=T + F)
    assert (ref["state_counts"].sum(1) == T * F).all()
    assert (ref["track_id"] >= 0).sum() == ref["track_length"].sum() == ref["state_counts"][:, [track.MATCHED, track.BORN]].sum()
    assert ref["num_tracks"].sum() == ref["state_counts"][:, track.BORN].sum()
    for s in range(S):                                             # the sequences are independent
        rows = slice(s * F, (s + 1) * F)
        alone = track.reference_associate(case["what"][:, rows], case["boxes"][:, rows], case["score"][:, rows], case["n"][rows], F)
        for k in ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot"):
            assert np.array_equal(alone[k], ref[k][:, rows], equal_nan=True), k
        assert np.array_equal(alone["track_gaps"][0], ref["track_gaps"][s])


def test_crafted_rows_reach_every_state_but_overflow():
    total = np.zeros(6, np.int64)
    for (T, A, S, F) in [(3, 5, 3, 5), (6, 50, 3, 17)]:
        total += crafted_rows(T, A, S, F, seed=T + A + S + F)[1]["state_counts"].sum(0)
    assert (total[[track.ABSENT, track.MATCHED, track.BORN, track.UNCONFIRMED, track.NONFINITE]] > 0).all()


# ---- reference_score ------------------------------------------------------------------------------------------------------------------
def score_case(ids, boxes_per_frame, gt_per_frame, T=2, tau=0.5):
    """one sequence: ids / boxes_per_frame [F][<= T], gt_per_frame [F][G] (None = absent)"""
    F, G = len(ids), len(gt_per_frame[0])
    boxes, tid, n, gt = np.zeros((T, F, 4), np.float32), np.full((T, F), -1, np.int32), np.zeros(F, np.int32), np.zeros((F, G, 4), np.float32)
    for f in range(F):
        n[f] = len(ids[f])
        for j, (i, b) in enumerate(zip(ids[f], boxes_per_frame[f])):
            tid[j, f], boxes[j, f] = i, b
        for g, b in enumerate(gt_per_frame[f]):
            if b is not None:
                gt[f, g] = b
    out = track.reference_score(boxes, n, tid, gt, F, tau)
    return out, track.mot_summary(out["seq_counts"][0], out["seq_iou"][0])


def test_a_perfect_track_scores_mota_one():
    P, Q = BOX(0.0), BOX(30.0)
    out, s = score_case([[0, 1]] * 4, [[P, Q]] * 4, [[P, Q]] * 4)
    assert out["seq_counts"][0].tolist() == [8, 8, 0, 0, 0, 2, 0, 2] and out["seq_iou"][0] == 8.0
    assert s["mota"] == 1.0 and s["motp"] == 1.0 and s["id_switches"] == 0 and s["mostly_tracked"] == 1.0 and s["mostly_lost"] == 0.0
    assert out["gt_match"].tolist() == [[0, 1]] * 4


def test_swapping_two_identities_once_counts_two_switches():
    P, Q = BOX(0.0), BOX(30.0)
    out, s = score_case([[0, 1], [0, 1], [1, 0], [1, 0]], [[P, Q]] * 4, [[P, Q]] * 4)
    assert out["seq_counts"][0].tolist() == [8, 8, 0, 0, 2, 2, 0, 2] and s["id_switches"] == 2 and s["mota"] == 1.0 - 2.0 / 8.0


def test_a_track_that_dies_and_is_reborn_counts_one_switch():
    P = BOX(0.0)
    out, s = score_case([[0], [0], [], [1], [1]], [[P], [P], [], [P], [P]], [[P]] * 5, T=1)
    assert out["seq_counts"][0].tolist() == [5, 4, 1, 0, 1, 1, 0, 1] and s["mota"] == 1.0 - 2.0 / 5.0
    assert out["gt_match"][:, 0].tolist() == [0, 0, -1, 0, 0]


def test_the_remembered_track_keeps_a_match_that_greedy_iou_would_reassign():
    P, near, exact = BOX(0.0), BOX(2.0), BOX(0.0)
    assert 0.5 < box_iou(P, near) < box_iou(P, exact)
    out, s = score_case([[5], [5, 7]], [[P], [near, exact]], [[P], [P]])
    assert out["gt_match"][:, 0].tolist() == [0, 0] and out["seq_counts"][0].tolist() == [2, 2, 0, 1, 0, 1, 0, 1]
    assert out["seq_iou"][0] == 1.0 + box_iou(P, near)
    out, _ = score_case([[6], [5, 7]], [[P], [near, exact]], [[P], [P]])      # nothing remembered in frame 1: greedy takes the better box
    assert out["gt_match"][:, 0].tolist() == [0, 1] and out["seq_counts"][0, 4] == 1
    out, _ = score_case([[5], [5, 7]], [[P], [BOX(6.0), exact]], [[P], [P]])   # the remembered track drifted below tau: reassigned
    assert out["gt_match"][:, 0].tolist() == [0, 1] and out["seq_counts"][0, 4] == 1


def test_mostly_tracked_and_mostly_lost_at_their_boundaries():
    P, far = BOX(0.0), BOX(300.0)
    for tracked, present, want in ((4, 5, (1, 0)), (3, 5, (0, 0)), (1, 5, (0, 1)), (2, 5, (0, 0)), (8, 10, (1, 0)), (7, 10, (0, 0)),
                                   (2, 10, (0, 1)), (3, 10, (0, 0))):
        ids = [[0]] * present
        boxes = [[P]] * tracked + [[far]] * (present - tracked)
        out, s = score_case(ids, boxes, [[P]] * present, T=1)
        assert (out["seq_counts"][0, 5], out["seq_counts"][0, 6]) == want, (tracked, present)
        assert out["seq_counts"][0, [0, 1, 2, 3, 7]].tolist() == [present, tracked, present - tracked, present - tracked, 1]


def test_an_empty_sequence_gives_nan():
    out, s = score_case([[], []], [[], []], [[None], [None]], T=1)
    assert out["seq_counts"][0].tolist() == [0] * 8 and out["seq_iou"][0] == 0.0
    assert all(np.isnan(s[k]) for k in ("mota", "motp", "mostly_tracked", "mostly_lost")) and s["id_switches"] == 0
    out, s = score_case([[3]], [[BOX(0.0)]], [[None]], T=1)        # hypotheses without ground truth: false positives, no rate
    assert out["seq_counts"][0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and np.isnan(s["mota"]) and s["false_positives"] == 1


def test_objects_without_an_id_or_with_a_nonfinite_box_are_no_hypotheses():
    P = BOX(0.0)
    out, _ = score_case([[-1, 2]], [[P, (np.nan, 0.0, 10.0, 10.0)]], [[P]])
    assert out["seq_counts"][0].tolist() == [1, 0, 1, 0, 0, 0, 1, 1] and out["gt_match"][0, 0] == -1


# ---- check_arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [(dict(iou_gate=1.0), "iou_gate"), (dict(iou_gate=-0.1), "iou_gate"), (dict(iou_gate=float("nan")), "iou_gate"),
                                      (dict(appearance_weight=1.5), "appearance_weight"), (dict(appearance_weight=-1e-9), "appearance_weight"),
                                      (dict(birth_score=2.0), "birth_score"), (dict(birth_score=float("nan")), "birth_score"),
                                      (dict(max_age=-1), "max_age"), (dict(max_age=1.5), "max_age"), (dict(max_steps=0), "max_steps"),
                                      (dict(max_steps=33), "max_steps"), (dict(n_frames=0), "n_frames"),
                                      (dict(max_steps=32, n_frames=1024, n_rows=1024), "int16"), (dict(n_rows=7), "multiple"),
                                      (dict(n_rows=0), "multiple")])
def test_check_arguments_refuses(kw, match):
    args = dict(max_steps=3, n_frames=4, n_rows=8)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        track.check_arguments(**args)


def test_check_arguments_accepts_the_limits():
    assert track.check_arguments(32, 1023, 2046, 0.0, 0.0, 0.0, 0) == (32, 1023, 2)
    assert track.check_arguments(1, 32767, None, 0.999, 1.0, 1.0, 100) == (1, 32767, None)
    assert track.check_arguments(3, 4, 8) == (3, 4, 2)


# ---- create_moving_mnist --------------------------------------------------------------------------------------------------------------
def disc_templates():
    yy, xx = np.mgrid[0:28, 0:28]
    return np.stack([(255 * np.clip(r - np.hypot(yy - 14, xx - 14), 0, 1)).astype(np.uint8) for r in (4, 5, 6, 7)])


def test_moving_mnist_is_deterministic_and_annotated_consistently():
    kw = dict(n_sequences=6, n_frames=9, canvas_size=(40, 50), n_objects=(0, 3), seed=3, return_annotations=True)
    a, b = create_moving_mnist(disc_templates(), **kw), create_moving_mnist(disc_templates(), **kw)
    assert all(np.array_equal(a[k], b[k]) for k in a) and set(a) == {"imgs", "nums", "boxes", "instances"}
    assert a["imgs"].shape == (6, 9, 40, 50) and a["imgs"].dtype == np.uint8 and a["instances"].dtype == np.int8
    assert a["boxes"].shape == (6, 9, 3, 4) and a["boxes"].dtype == np.float32 and a["nums"].shape == (6, 9)
    c = create_moving_mnist(disc_templates(), **dict(kw, seed=4))
    assert not np.array_equal(a["imgs"], c["imgs"])
    plain = create_moving_mnist(disc_templates(), **dict(kw, return_annotations=False))
    assert set(plain) == {"imgs", "nums"} and np.array_equal(plain["imgs"], a["imgs"])
    boxes, inst = a["boxes"], a["instances"]
    present = boxes[..., 2] > 0
    assert np.array_equal(a["nums"], present.sum(-1)) and a["nums"].max() == 3 and (a["nums"].min(1) == a["nums"].max(1)).all()
    assert (boxes[present][:, 0] >= 0).all() and (boxes[present][:, 1] >= 0).all()
    assert (boxes[present][:, 0] + boxes[present][:, 2] <= 50).all() and (boxes[present][:, 1] + boxes[present][:, 3] <= 40).all()
    assert ((inst >= 0) == (a["imgs"] > 0)).all()
    moved, checked = 0, 0
    for s in range(6):
        for j in range(3):
            if not present[s, 0, j]:
                assert not present[s, :, j].any()
                continue
            assert (boxes[s, :, j, 2:] == boxes[s, 0, j, 2:]).all()              # the same template over the sequence
            moved += int((boxes[s, 1:, j, :2] != boxes[s, :-1, j, :2]).any())
            step = np.abs(np.diff(boxes[s, :, j, :2], axis=0))
            assert (np.hypot(step[:, 0], step[:, 1]) <= 3.0 + 1.5).all()          # speed <= 3, two roundings
            for f in range(9):
                l, t, w, h = (int(v) for v in boxes[s, f, j])
                others = [k for k in range(3) if k != j and present[s, f, k]]
                if any(box_iou(boxes[s, f, j], boxes[s, f, k]) > 0 for k in others):
                    continue                                       # (occluded or occluding: the bounds need not be tight)
                ys, xs = np.nonzero(inst[s, f] == j)
                assert (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) == (l, t, w, h)
                checked += 1
    assert moved > 0 and checked > 20


def test_moving_mnist_higher_slot_wins_an_overlap_and_pixels_take_the_maximum():
    full = create_moving_mnist(np.stack([disc_templates()[3]] * 2), 8, 3, canvas_size=(16, 16), n_objects=2, speed=(0.0, 0.0), seed=2,
                               return_annotations=True)
    both = np.flatnonzero((full["boxes"][:, 0, :, 2] > 0).all(1))
    assert both.size > 0
    for s in both:
        assert (full["boxes"][s, 0] == full["boxes"][s, 2]).all()                # speed 0: nothing moves
        (l0, t0, w, h), (l1, t1, _, _) = (tuple(int(v) for v in b) for b in full["boxes"][s, 0])
        crop = full["imgs"][s, 0, t1:t1 + h, l1:l1 + w]
        assert (full["instances"][s, 0, t1:t1 + h, l1:l1 + w][crop > 0] >= 0).all()
        inside = full["instances"][s, 0, t1:t1 + h, l1:l1 + w]
        template = _tight_box(disc_templates()[3])
        (y0, x0), (sh, sw) = template
        ink = disc_templates()[3][y0:y0 + sh, x0:x0 + sw]
        assert (inside[ink > 0] == 1).all()                        # slot 1 owns every pixel of its own ink
        canvas = np.zeros((16, 16), np.uint8)
        for (l, t) in ((l0, t0), (l1, t1)):
            canvas[t:t + sh, l:l + sw] = np.maximum(canvas[t:t + sh, l:l + sw], ink)
        assert np.array_equal(canvas, full["imgs"][s, 0])


def test_bounce_reflects_off_both_edges_by_hand():
    assert _bounce(3.0, 2.5, np.arange(6), 10).tolist() == [3.0, 5.5, 8.0, 9.5, 7.0, 4.5]
    assert _bounce(1.0, -2.0, np.arange(4), 10).tolist() == [1.0, 1.0, 3.0, 5.0]
    assert _bounce(4.0, 7.0, np.arange(5), 10).tolist() == [4.0, 9.0, 2.0, 5.0, 8.0]      # 11 -> 9, 18 -> 2, 25 -> 5 (two edges), 32 -> 8
    assert _bounce(0.0, 3.0, np.arange(3), 0).tolist() == [0.0, 0.0, 0.0]
    # through the generator: one template that fills a 10 x 10 box on a 10 x 30 canvas can only move along x
    templates = np.zeros((1, 28, 28), np.uint8)
    templates[0, 5:15, 5:15] = 255
    d = create_moving_mnist(templates, 1, 40, canvas_size=(10, 30), n_objects=1, speed=(4.0, 4.0), seed=1, return_annotations=True)
    assert d["nums"].sum() in (0, 40)
    d = next(x for x in (create_moving_mnist(templates, 1, 40, canvas_size=(10, 30), n_objects=1, speed=(4.0, 4.0), seed=k,
                                             return_annotations=True) for k in range(20)) if x["nums"].sum())
    x = d["boxes"][0, :, 0, 0]
    assert (d["boxes"][0, :, 0, 1] == 0).all() and x.min() >= 0 and x.max() <= 20
    rs = np.random.RandomState(next(k for k in range(20) if create_moving_mnist(templates, 1, 1, canvas_size=(10, 30), n_objects=1,
                                                                                seed=k)["nums"].sum()))
    assert rs.randint(2, size=1)[0] == 1 and rs.choice(1, 1, replace=False)[0] == 0        # the documented order of draws, replayed
    start, theta, u = rs.rand(2) * np.array([0.0, 20.0]), 2.0 * np.pi * rs.rand(), rs.rand()
    want = np.round(_bounce(start[1], (4.0 + u * 0.0) * np.cos(theta), np.arange(40), 20))
    assert np.array_equal(x, want.astype(np.float32)) and np.abs(np.diff(np.sign(np.diff(x)))).max() > 0      # it did turn round


def test_moving_mnist_spans_produce_births_and_deaths():
    d = create_moving_mnist(disc_templates(), 16, 8, n_objects=(0, 2), spans=True, seed=5, return_annotations=True)
    present = d["boxes"][..., 2] > 0
    assert np.array_equal(d["nums"], present.sum(-1))
    used = present.any(1)
    assert used.any() and (~present[used.nonzero()[0]]).any()      # absent rows inside sequences that have the object
    for s, j in zip(*used.nonzero()):
        on = np.flatnonzero(present[s, :, j])
        assert np.array_equal(on, np.arange(on[0], on[-1] + 1))    # one interval
        assert (d["boxes"][s, ~present[s, :, j], j] == 0).all()
    assert any(np.flatnonzero(present[s, :, j])[0] > 0 for s, j in zip(*used.nonzero()))
    assert any(np.flatnonzero(present[s, :, j])[-1] < 7 for s, j in zip(*used.nonzero()))


def test_procedural_moving_mnist():
    d = procedural_moving_mnist(3, 4, n_objects=(0, 2), seed=1, n_templates=16, return_annotations=True)
    assert d["imgs"].shape == (3, 4, 50, 50) and d["boxes"].shape == (3, 4, 2, 4) and d["imgs"].max() > 0
    e = procedural_moving_mnist(3, 4, n_objects=(0, 2), seed=1, n_templates=16, return_annotations=True)
    assert all(np.array_equal(d[k], e[k]) for k in d)
    with pytest.raises(ValueError, match="speed"):
        procedural_moving_mnist(1, 2, speed=(3.0, 1.0), n_templates=4)
