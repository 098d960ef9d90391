"""Host-side tests of stream tracking (attend_infer_repeat_amd/track.py): chunk invariance of `reference_associate_stream` against the
one-shot `reference_associate` under every chunking and both matchings, padding that must not matter, the boundary cases written out
by hand, the id limit, `reference_score_stream`, and the refusals.  No GPU.  Every comparison is exact (affinity by bits)."""
import types

import numpy as np
import pytest

from test_track_host import BOX, CROSSING, build_rows, moving_gt, score_case
from track_stream_cases import (HOST_PARAMS, ROWS, assemble, bits, check_against_one_shot, check_written, chunkings, cut, one_shot,
                                reference_stream, same, states_equal)

from attend_infer_repeat_amd import track


# ---- chunk invariance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("T,A,S,F_total", HOST_PARAMS)
def test_any_chunking_is_the_one_shot_rule(T, A, S, F_total, matching):
    kw = dict(iou_gate=0.2, appearance_weight=0.6, birth_score=0.4, max_age=2) if (T + A) % 2 else {}
    case, ref = one_shot(T, A, S, F_total, matching, **kw)
    names = []
    for name, F, valids in chunkings(S, F_total):
        chunks = cut(case, F, valids)
        outs, states = reference_stream(chunks, matching)
        for o, c in zip(outs, chunks):
            check_written(o, c)
        check_against_one_shot(assemble(outs, chunks), states[-1], case, matching)
        names.append(name)
    assert names == ["ones", "one", "twos", "fours", "ragged"]
    assert ref["state_counts"][:, [track.MATCHED, track.BORN]].sum() > 0


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_padding_rows_do_not_matter(matching):
    case, _ = one_shot(3, 5, 3, 6, matching)
    name, F, valids = chunkings(3, 6)[-1]
    base_outs, base_states = reference_stream(cut(case, F, valids, "zero"), matching)
    for pad in ("nan", "garbage"):
        chunks = cut(case, F, valids, pad, seed=5)
        assert any(np.isnan(c["what"]).any() or (c["n"] == 99).any() for c in chunks)
        outs, states = reference_stream(chunks, matching)
        for o, b in zip(outs, base_outs):
            assert set(o) == set(b) and all(same(o[k], b[k]) for k in o)
        for x, y in zip(states, base_states):
            states_equal(x, y)


def test_the_input_state_is_not_modified_and_none_starts_a_stream():
    case, _ = one_shot(3, 5, 3, 6, "greedy")
    chunks = cut(case, 2, chunkings(3, 6)[2][2])
    out0, st0 = track.reference_associate_stream(None, chunks[0]["what"], chunks[0]["boxes"], chunks[0]["score"], chunks[0]["n"], 2)
    keep = {k: v.copy() for k, v in st0.items()}
    track.reference_associate_stream(st0, chunks[1]["what"], chunks[1]["boxes"], chunks[1]["score"], chunks[1]["n"], 2)
    states_equal(st0, keep)
    fresh = track.new_stream_state(3, 5)
    assert (fresh["seq"] == 0).all() and (fresh["slots"][:, track.ST_LIVE] == 0).all() and (fresh["slots"][:, track.ST_ID] == -1).all()
    assert set(st0) == set(track.STATE_KEYS) and st0["what"].shape == (3, 32, 5) and st0["slots"].shape == (3, 8, 32)


# ---- written out by hand ----------------------------------------------------------------------------------------------------------------
def stream(frames_per_chunk, T, F, A=2, state=None, valid=None, **kw):
    """push hand-written chunks (each a list of F frames for ONE sequence) through the reference; returns (outs, state)"""
    outs = []
    for i, frames in enumerate(frames_per_chunk):
        what, boxes, score, n = build_rows(frames, T, A)
        out, state = track.reference_associate_stream(state, what, boxes, score, n, F, None if valid is None else valid[i], **kw)
        outs.append(out)
    return outs, state


def test_a_track_is_matched_across_the_boundary_with_a_global_prev_frame():
    P = lambda x: (BOX(x), 0.9, 1.0)
    outs, state = stream([[[], [P(0.0)]], [[P(1.0)], [P(2.0)]]], 1, 2)
    assert outs[0]["track_id"][0].tolist() == [-1, 0] and outs[0]["obj_state"][0].tolist() == [track.ABSENT, track.BORN]
    assert outs[1]["track_id"][0].tolist() == [0, 0] and outs[1]["obj_state"][0].tolist() == [track.MATCHED] * 2
    assert outs[1]["prev_frame"][0].tolist() == [1, 2] and outs[1]["prev_slot"][0].tolist() == [0, 0]       # frame 1 is chunk 0's last
    assert outs[1]["num_retired"].tolist() == [0] and state["seq"][0].tolist() == [4, 1]
    assert track.stream_live(state)[0] == [dict(slot=0, id=0, first=1, last=3, length=3, gaps=0, age=0)]
    assert state["box"][0, 0].tolist() == list(BOX(2.0)) and state["what"][0, 0].tolist() == [1.0, 1.0]


def test_an_object_missing_in_the_last_frame_of_a_chunk_returns_under_its_id():
    P = lambda x: (BOX(x), 0.9, 1.0)
    outs, state = stream([[[P(0.0)], []], [[P(1.0)], []]], 2, 2, max_age=1)
    assert outs[0]["track_id"][0].tolist() == [0, -1] and outs[1]["track_id"][0].tolist() == [0, -1]
    assert outs[1]["obj_state"][0, 0] == track.MATCHED and outs[1]["prev_frame"][0, 0] == 0 and outs[1]["prev_slot"][0, 0] == 0
    (t,) = track.stream_live(state)[0]
    assert (t["id"], t["first"], t["last"], t["length"], t["gaps"], t["age"]) == (0, 0, 2, 2, 1, 1)
    assert outs[0]["num_retired"].tolist() == [0] and outs[1]["num_retired"].tolist() == [0]


def test_an_object_missing_max_age_plus_one_frames_across_the_boundary_gets_a_new_id():
    P = lambda x: (BOX(x), 0.9, 1.0)
    outs, state = stream([[[P(0.0)], [P(0.0)], []], [[], [P(0.0)], [P(0.0)]]], 1, 3, max_age=1)
    assert outs[0]["track_id"][0].tolist() == [0, 0, -1] and outs[0]["num_retired"].tolist() == [0]
    assert outs[1]["track_id"][0].tolist() == [-1, 1, 1] and outs[1]["obj_state"][0].tolist() == [track.ABSENT, track.BORN, track.MATCHED]
    assert outs[1]["num_retired"].tolist() == [1]                  # retired in frame 3, the first of chunk 1, with its GLOBAL last frame
    assert [int(outs[1][k][0, 0]) for k in track.RETIRED] == [0, 0, 1, 2, 0]
    assert all(int(outs[1][k][0, 1]) == e for k, e in zip(track.RETIRED, (-1, -1, -1, 0, 0)))
    (t,) = track.stream_live(state)[0]
    assert (t["id"], t["first"], t["last"], t["length"]) == (1, 4, 5, 2) and outs[1]["prev_frame"][0, 2] == 4


def test_crossing_at_the_boundary_follows_the_what_code_of_the_state():
    for w, swapped in ((0.0, True), (0.5, False)):
        outs, state = stream([[CROSSING[0]], [CROSSING[1]]], 2, 1, iou_gate=0.1, appearance_weight=w)
        assert outs[0]["track_id"][:, 0].tolist() == [0, 1]
        assert outs[1]["track_id"][:, 0].tolist() == ([1, 0] if swapped else [0, 1])
        assert outs[1]["obj_state"][:, 0].tolist() == [track.MATCHED] * 2 and outs[1]["prev_frame"][:, 0].tolist() == [0, 0]
        assert outs[1]["prev_slot"][:, 0].tolist() == ([1, 0] if swapped else [0, 1])
        what, boxes, score, n = build_rows(CROSSING, 2)
        ref = track.reference_associate(what, boxes, score, n, 2, iou_gate=0.1, appearance_weight=w)
        assert np.array_equal(bits(outs[1]["affinity"][:, 0]), bits(ref["affinity"][:, 1]))
    # the code comes from the state and from nowhere else: with the state's copies exchanged the ids follow them
    (out0,), state = stream([[CROSSING[0]]], 2, 1, iou_gate=0.1, appearance_weight=0.5)
    state["what"][0, [0, 1]] = state["what"][0, [1, 0]]
    (out1,), _ = stream([[CROSSING[1]]], 2, 1, state=state, iou_gate=0.1, appearance_weight=0.5)
    assert out1["track_id"][:, 0].tolist() == [1, 0]


def test_ids_stop_at_32766():
    P = lambda x, y=0.0: ((x, y, 10.0, 10.0), 0.9, 1.0)
    state = track.new_stream_state(1, 2)
    state["seq"][0] = (100, 32766)
    (out,), state = stream([[[P(0.0), P(100.0)]]], 2, 1, state=state)
    assert out["track_id"][:, 0].tolist() == [32766, -1] and out["obj_state"][:, 0].tolist() == [track.BORN, track.OVERFLOW]
    assert state["seq"][0].tolist() == [101, 32767] and out["state_counts"][0].tolist() == [0, 0, 1, 0, 1, 0]
    (out,), state = stream([[[P(1.0), P(101.0)]]], 2, 1, state=state)           # the live track goes on; nothing is born any more
    assert out["track_id"][:, 0].tolist() == [32766, -1] and out["obj_state"][:, 0].tolist() == [track.MATCHED, track.OVERFLOW]
    assert out["prev_frame"][0, 0] == 100 and state["seq"][0].tolist() == [102, 32767]


def test_reset_restarts_one_sequence_alone():
    case, _ = one_shot(3, 5, 3, 6, "greedy")
    chunks = cut(case, 2, chunkings(3, 6)[2][2])
    outs, states = reference_stream(chunks[:2], "greedy")
    state = {k: v.copy() for k, v in states[-1].items()}
    assert state["seq"][1, 1] > 0 and state["slots"][1, track.ST_LIVE].any()
    track.reset_stream_state(state, [1])
    fresh = track.new_stream_state(3, 5)
    for k in track.STATE_KEYS:
        assert same(state[k][1], fresh[k][1]) and same(state[k][[0, 2]], states[-1][k][[0, 2]]), k
    # sequence 1 now tracks chunk 2 as a stream of its own, the others go on
    out, after = track.reference_associate_stream(state, *(chunks[2][k] for k in ("what", "boxes", "score", "n")), 2)
    alone, _ = track.reference_associate_stream(None, *(chunks[2][k][:, 2:4] if k != "n" else chunks[2][k][2:4]
                                                        for k in ("what", "boxes", "score", "n")), 2)
    cont, _ = track.reference_associate_stream(states[-1], *(chunks[2][k] for k in ("what", "boxes", "score", "n")), 2)
    for k in ROWS:
        assert same(out[k][:, 2:4], alone[k]) and same(out[k][:, [0, 1, 4, 5]], cont[k][:, [0, 1, 4, 5]]), k
    assert after["seq"][1, 0] == 2 and after["seq"][0, 0] == 6
    with pytest.raises(ValueError, match="sequences"):
        track.reset_stream_state(state, [3])


# ---- score ------------------------------------------------------------------------------------------------------------------------------
def score_stream(case, ids, gt, F, valids, tau=0.5, pad_ids=77):
    """reference_score_stream over the chunks of a one-shot case (boxes, n, ids, gt): the last outputs and every chunk's gt_match"""
    S, Ft, T, G = case["S"], case["F"], case["T"], gt.shape[1]
    at, state, matches = np.zeros(S, np.int64), None, [[] for _ in range(S)]
    for v in valids:
        R = S * F
        boxes, n, tid, g = np.full((T, R, 4), np.nan, np.float32), np.full(R, 99, np.int32), np.full((T, R), pad_ids, np.int32), np.ones((R, G, 4), np.float32)
        for s in range(S):
            src, dst = slice(s * Ft + at[s], s * Ft + at[s] + v[s]), slice(s * F, s * F + v[s])
            boxes[:, dst], n[dst], tid[:, dst], g[dst] = case["boxes"][:, src], case["n"][src], ids[:, src], gt[src]
        out, state = track.reference_score_stream(state, boxes, n, tid, g, F, v, tau)
        for s in range(S):
            matches[s].append(out["gt_match"][s * F:s * F + int(v[s])])
            assert (out["gt_match"][s * F + int(v[s]):(s + 1) * F] == -1).all()
        at = at + v
    return out, np.concatenate([np.concatenate(m) for m in matches]), state


@pytest.mark.parametrize("T,S,F_total,G,tau", [(3, 3, 6, 1, 0.5), (3, 3, 6, 8, 0.5), (6, 2, 15, 8, 0.3), (32, 1, 6, 8, 0.5)])
def test_score_stream_is_the_one_shot_score(T, S, F_total, G, tau):
    case, ref = one_shot(T, 5, S, F_total, "greedy")
    rng = np.random.default_rng(T + G)
    gt = moving_gt(case, rng, G)
    ids = ref["track_id"].copy()
    flip = rng.uniform(size=ids.shape) < 0.1
    ids[flip & (ids >= 0)] += 1
    want = track.reference_score(case["boxes"], case["n"], ids, gt, F_total, tau)
    assert want["seq_counts"][:, 0].sum() > 0
    for name, F, valids in chunkings(S, F_total):
        out, gm, _ = score_stream(case, ids, gt, F, valids, tau)
        assert np.array_equal(out["seq_counts"], want["seq_counts"]), name
        assert np.array_equal(out["seq_iou"].view(np.uint64), want["seq_iou"].view(np.uint64)), name      # continued, not re-added
        assert np.array_equal(gm, want["gt_match"]), name


def test_an_identity_switch_at_the_boundary_counts_in_the_stream_only():
    P = BOX(0.0)
    ids, boxes, gt = [[0], [0], [1], [1]], [[P]] * 4, [[P]] * 4
    whole, _ = score_case(ids, boxes, gt, T=1)
    assert whole["seq_counts"][0, 4] == 1
    halves = [score_case(ids[i:i + 2], boxes[i:i + 2], gt[i:i + 2], T=1)[0] for i in (0, 2)]
    assert [h["seq_counts"][0, 4] for h in halves] == [0, 0]       # scored separately the switch is invisible
    state = None
    for i in (0, 2):
        b, t, n, g = np.zeros((1, 2, 4), np.float32), np.zeros((1, 2), np.int32), np.ones(2, np.int32), np.zeros((2, 1, 4), np.float32)
        b[0, :], g[:, 0], t[0] = P, P, [ids[i][0], ids[i + 1][0]]
        out, state = track.reference_score_stream(state, b, n, t, g, 2)
    assert out["seq_counts"][0].tolist() == whole["seq_counts"][0].tolist() == [4, 4, 0, 0, 1, 1, 0, 1]
    assert state["score_i"][0, 8] == 1 and state["score_i"][0, 4] == 1


def test_mostly_tracked_and_lost_thresholds_over_two_chunks():
    P, far = BOX(0.0), BOX(300.0)
    for tracked, present, want in ((4, 5, (1, 0)), (3, 5, (0, 0)), (1, 5, (0, 1)), (2, 5, (0, 0)), (8, 10, (1, 0)), (7, 10, (0, 0)),
                                   (2, 10, (0, 1)), (3, 10, (0, 0))):
        F, state = present // 2 + 1, None                         # two chunks: F frames, then the rest (ragged, with padding)
        hyp = [P] * tracked + [far] * (present - tracked)
        for lo, hi in ((0, F), (F, present)):
            b, t, n, g = np.zeros((1, F, 4), np.float32), np.zeros((1, F), np.int32), np.ones(F, np.int32), np.zeros((F, 1, 4), np.float32)
            b[0, :hi - lo], g[:hi - lo, 0] = hyp[lo:hi], P
            out, state = track.reference_score_stream(state, b, n, t, g, F, np.array([hi - lo]))
        assert (out["seq_counts"][0, 5], out["seq_counts"][0, 6]) == want, (tracked, present)
        assert out["seq_counts"][0, [0, 1, 2, 3, 7]].tolist() == [present, tracked, present - tracked, present - tracked, 1]
        assert state["score_i"][0, 16] == tracked and state["score_i"][0, 24] == present


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    case, _ = one_shot(3, 5, 3, 6, "greedy")
    c = cut(case, 2, chunkings(3, 6)[2][2])[0]
    args = (c["what"], c["boxes"], c["score"], c["n"], 2)
    for bad in (np.zeros(2, np.int64), np.zeros((3, 1), np.int64), np.zeros(3, np.float32), [1, 2]):
        with pytest.raises(ValueError, match="valid"):
            track.reference_associate_stream(None, *args, bad)
        with pytest.raises(ValueError, match="valid"):
            track.check_valid(bad, 3, 2)
    assert track.check_valid([5, -1, 1], 3, 2).tolist() == [2, 0, 1] and track.check_valid(None, 3, 2).tolist() == [2, 2, 2]
    with pytest.raises(ValueError, match="int16"):                 # chunk_frames * T ids must fit int16, as for the one-shot tracker
        track.check_arguments(32, 1024, 1024)
    big = dict(what=np.zeros((32, 1024, 1), np.float32), boxes=np.zeros((32, 1024, 4), np.float32), score=np.zeros((32, 1024), np.float32))
    with pytest.raises(ValueError, match="int16"):
        track.reference_associate_stream(None, big["what"], big["boxes"], big["score"], np.zeros(1024, np.int32), 1024)
    with pytest.raises(ValueError, match="matching"):
        track.reference_associate_stream(None, *args, matching="best")
    with pytest.raises(ValueError, match="ParticleParser"):
        track.StreamTracker(types.SimpleNamespace(KIND="particle", engine=None, R=10, T=3), 5)
    assert track.StreamTracker.REFUSALS is track.SequenceTracker.REFUSALS and track.StreamTracker.ACCEPTS == track.SequenceTracker.ACCEPTS
    state = track.new_stream_state(3, 5)
    state["seq"][1, 0] = 2 ** 31 - 2
    with pytest.raises(ValueError, match="frames_seen"):
        track.reference_associate_stream(state, *args)
    out, after = track.reference_associate_stream(state, *args, np.array([2, 1, 2]))      # exactly to the limit is fine
    assert after["seq"][1, 0] == 2 ** 31 - 1
    with pytest.raises(ValueError, match="frames_seen"):
        track.check_frames_seen(np.array([0, 2 ** 31 - 1]), np.array([2, 1]))
    with pytest.raises(ValueError, match="sequences"):
        track.reference_associate_stream(track.new_stream_state(2, 5), *args)
