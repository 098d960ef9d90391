"""Cases shared by test_track_stream_host.py and test_track_stream.py: how a one-shot case is cut into the chunks of a stream (the
chunkings, the padding fills), how the chunk outputs are put together again, and the one-shot answer they are compared with.

Everything is compared exactly.  The inputs are those of crafted_rows / crafted_optimal / full_table_rows, with MARGIN asserted on the
one-shot reference: the stream takes the same decisions on the same numbers (a track's last-sighting box and `what` row are bit
copies), so the margins carry over to every chunking."""
import numpy as np

from test_track_host import crafted_rows
from track_optimal_cases import MARGIN, crafted_optimal, full_table_rows

from attend_infer_repeat_amd import track

ROWS = ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot")
HOST_PARAMS = [(1, 1, 1, 3), (3, 5, 3, 6), (6, 50, 2, 15), (32, 5, 1, 6)]
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """two arrays of any type: the same type, shape and bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def one_shot(T, A, S, F_total, matching, seed=None, **kw):
    """(case, one-shot reference) of crafted rows under `matching`, the margins asserted"""
    seed = T + A + S + F_total if seed is None else seed
    if matching == "optimal":
        case, ref = crafted_optimal(T, A, S, F_total, seed=seed, **kw)
    else:
        case, ref = crafted_rows(T, A, S, F_total, seed=seed, margin=MARGIN, **kw)
        assert (ref["round_margin"] >= MARGIN).all()
    assert (ref["gate_margin"] >= MARGIN).all()
    return case, ref


def full_table_case(matching, F_total=6, A=5):
    """full_table_rows (T = 32, all 32 slots live from frame 0 on, S = 1) at the first seed whose one-shot decisions are MARGIN from
    flipping; gate 0: every pair is admissible"""
    kw = dict(iou_gate=0.0, appearance_weight=0.5)
    for seed in range(50):
        case = full_table_rows(A=A, F=F_total, seed=seed)
        ref = track.reference_associate(case["what"], case["boxes"], case["score"], case["n"], F_total, return_margins=True,
                                        matching=matching, **kw)
        if (ref["gate_margin"] >= MARGIN).all() and (matching == "optimal" or (ref["round_margin"] >= MARGIN).all()):
            case["kw"] = kw
            assert ref["num_tracks"][0] == 32 and (ref["track_length"][0, :32] == F_total).all()      # every slot live throughout
            return case, ref
    raise AssertionError("no full table within the margins")


def chunkings(S, F_total):
    """[(name, chunk_frames, [valid [S] per chunk])]: all-ones chunks, one chunk, chunks of 2, chunks of 4 with a ragged last one, and
    per-sequence different counts with a valid = 0 chunk in the middle; every sequence gets all its F_total frames"""
    def even(F):
        return [np.full(S, min(F, F_total - at), np.int64) for at in range(0, F_total, F)]
    plans = [("ones", 1, even(1)), ("one", F_total, even(F_total)), ("twos", 2, even(2)), ("fours", 4, even(4))]
    F, left, valids = 3, np.full(S, F_total, np.int64), []
    while left.any():
        c = len(valids)
        want = np.array([0 if (c + s) % 3 == 1 else 1 + (c + 2 * s) % 3 for s in range(S)], np.int64)
        valids.append(np.minimum(want, left))
        left = left - valids[-1]
    assert any((v == 0).any() for v in valids[1:-1]) or F_total < 4
    plans.append(("ragged", F, valids))
    return plans


def cut(case, F, valids, pad="zero", seed=0):
    """the chunks of a stream over a one-shot case: per chunk the arrays as the kernel takes them at R = S * F rows, sequence s holding
    its next valid[s] frames and behind them padding filled by `pad`: "zero", "nan" (NaN rows, counts of 99) or "garbage" (random
    numbers of every size and sign, counts of 99)"""
    T, A, S, Ft = case["T"], case["A"], case["S"], case["F"]
    rng = np.random.default_rng(seed)
    at, chunks = np.zeros(S, np.int64), []
    for v in valids:
        R = S * F
        if pad == "zero":
            what, boxes, score, n = np.zeros((T, R, A), np.float32), np.zeros((T, R, 4), np.float32), np.zeros((T, R), np.float32), np.zeros(R, np.int32)
        elif pad == "nan":
            what, boxes, score = (np.full(shape, np.nan, np.float32) for shape in ((T, R, A), (T, R, 4), (T, R)))
            n = np.full(R, 99, np.int32)
        else:
            what, boxes, score = ((rng.normal(size=shape) * 10.0 ** rng.integers(-3, 6, shape)).astype(np.float32)
                                  for shape in ((T, R, A), (T, R, 4), (T, R)))
            n = np.full(R, 99, np.int32)
        for s in range(S):
            src, dst = slice(s * Ft + at[s], s * Ft + at[s] + v[s]), slice(s * F, s * F + v[s])
            what[:, dst], boxes[:, dst], score[:, dst], n[dst] = case["what"][:, src], case["boxes"][:, src], case["score"][:, src], case["n"][src]
        chunks.append(dict(what=what, boxes=boxes, score=score, n=n, valid=np.asarray(v, np.int64), T=T, A=A, S=S, F=F, kw=case["kw"]))
        at = at + v
    return chunks


def reference_stream(chunks, matching, state=None):
    """track.reference_associate_stream over the chunks: ([outputs per chunk], [state after each chunk])"""
    outs, states = [], []
    for c in chunks:
        out, state = track.reference_associate_stream(state, c["what"], c["boxes"], c["score"], c["n"], c["F"], c["valid"],
                                                      matching=matching, **c["kw"])
        outs.append(out)
        states.append(state)
    return outs, states


def assemble(outs, chunks):
    """the chunk outputs of a stream put together again, per sequence: rows {key: [T, frames fed]} (prev_frame global as the stream
    gives it), retired [(id, first, last, length, gaps)] in the order listed, counts [6]"""
    S, F = chunks[0]["S"], chunks[0]["F"]
    per = []
    for s in range(S):
        rows = {k: np.concatenate([o[k][:, s * F:s * F + int(c["valid"][s])] for o, c in zip(outs, chunks)], 1) for k in ROWS}
        retired = [tuple(int(o[k][s, i]) for k in track.RETIRED) for o in outs for i in range(int(o["num_retired"][s]))]
        per.append(dict(rows=rows, retired=retired, counts=sum(o["state_counts"][s].astype(np.int64) for o in outs)))
    return per


def check_written(out, chunk):
    """every element of a chunk's outputs has its stated value where nothing happened: the padding rows and the unused retired rows"""
    S, F, T = chunk["S"], chunk["F"], chunk["T"]
    for s in range(S):
        v, nr = int(chunk["valid"][s]), int(out["num_retired"][s])
        pad = slice(s * F + v, (s + 1) * F)
        assert (out["track_id"][:, pad] == -1).all() and (out["obj_state"][:, pad] == track.ABSENT).all()
        assert (bits(out["affinity"][:, pad]) == 0).all() and (out["prev_frame"][:, pad] == -1).all() and (out["prev_slot"][:, pad] == -1).all()
        assert out["state_counts"][s].sum() == T * v
        assert 0 <= nr <= 32 + F * T
        for k, empty in zip(track.RETIRED, (-1, -1, -1, 0, 0)):
            assert out[k].shape == (S, 32 + F * T) and (out[k][s, nr:] == empty).all() and (out[k][s, :nr] >= 0).all(), k


def check_against_one_shot(per, state, case, matching, fed=None):
    """chunk invariance: the assembled stream of every sequence against reference_associate on that sequence alone (S = 1, at the
    length fed): the [T, .] outputs exactly (affinity by bits; the stream's prev_frame is global, as the one-shot's is on one sequence
    from frame 0), the retired lists plus the live tracks against the per-id tables, the summed state_counts"""
    T, S, Ft = case["T"], case["S"], case["F"]
    live = track.stream_live(state)
    for s in range(S):
        n = Ft if fed is None else int(fed[s])
        src = slice(s * Ft, s * Ft + n)
        if n == 0:
            assert per[s]["rows"]["track_id"].shape[1] == 0 and not per[s]["retired"] and not live[s]
            continue
        ref = track.reference_associate(case["what"][:, src], case["boxes"][:, src], case["score"][:, src], case["n"][src], n,
                                        matching=matching, **case["kw"])
        for k in ROWS:
            got, want = per[s]["rows"][k], ref[k]
            assert got.dtype == want.dtype and got.shape == want.shape, k
            assert np.array_equal(bits(got), bits(want)) if k == "affinity" else np.array_equal(got, want), (k, s)
        assert np.array_equal(per[s]["counts"], ref["state_counts"][0])
        tracks = {t[0]: t[1:] for t in per[s]["retired"]}
        assert len(tracks) == len(per[s]["retired"])               # an id is retired once
        for t in live[s]:
            assert t["id"] not in tracks
            tracks[t["id"]] = (t["first"], t["last"], t["length"], t["gaps"])
        nt = int(ref["num_tracks"][0])
        assert sorted(tracks) == list(range(nt)) and int(state["seq"][s, 1]) == nt and int(state["seq"][s, 0]) == n
        for i in range(nt):
            assert tracks[i] == tuple(int(ref[k][0, i]) for k in ("track_first", "track_last", "track_length", "track_gaps")), (s, i)
        gone = [last + int(case["kw"].get("max_age", track.DEFAULTS["max_age"])) + 1 for (_, _, last, _, _) in per[s]["retired"]]
        assert gone == sorted(gone)                                # listed in ascending retirement frame


def states_equal(a, b):
    """two stream states, every array exactly (`what` and `box` by bits)"""
    for k in track.STATE_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y), k
