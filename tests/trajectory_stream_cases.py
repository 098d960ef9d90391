"""Cases shared by test_trajectory_stream_host.py and test_trajectory_stream.py: crafted tracker outputs (track.reference_associate on
crafted_rows / full_table_rows, with `where` and glimpse rows next to them), cut into the chunks of a stream; the one-shot answer on a
PREFIX of a sequence, which is what a fixed-lag smoother must reproduce; and what a case has to contain.

Everything is compared exactly, by bytes.  What a case contains is asserted on the host reference where the case can hold it: one
object per frame over three frames (1, 1, 1, 3) cannot both coast and retire a track, and the full table (32 tracks sighted in
every frame) neither coasts nor retires one, so `FEATURES` says per case what is asserted; the two middle cases hold everything."""
import functools

import numpy as np

from track_stream_cases import chunkings, full_table_case, one_shot, same

from attend_infer_repeat_amd import trajectory
from attend_infer_repeat_amd.trajectory import ABSENT, FILLED, OBSERVED

IMG = (50, 50)
G = 4
TABLE = ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity")
ROWS = ("what", "glimpse", "score")
NOISE = dict(process_noise=(2e-4, 5e-5), measurement_noise=3e-4, velocity_var=0.05)
# (T, A, S, F_total, max_age) -> what the case must contain
FEATURES = {(1, 1, 1, 3, 1): ("born_last",),
            (3, 5, 3, 6, 1): ("coasts_and_returns", "retired", "row_reused", "born_last"),
            (6, 50, 2, 15, 2): ("coasts_and_returns", "retired", "row_reused", "born_last"),
            (3, 50, 1, 6, 1): ("coasts_and_returns", "retired", "row_reused", "born_last"),
            (32, 5, 1, 6, 1): ("born_last",)}
HOST_PARAMS = [(1, 1, 1, 3, 1), (3, 5, 3, 6, 1), (6, 50, 2, 15, 2), (32, 5, 1, 6, 1)]


def prefix_tracks(track_id, n, T):
    """num_tracks [1], track_first, track_last [1, F T] of ONE sequence's ids [T, F]: what the (causal) tracker has written after
    these frames"""
    F = track_id.shape[1]
    first, last = np.full((1, F * T), -1, np.int32), np.full((1, F * T), -1, np.int32)
    for f in range(F):
        for j in range(int(np.clip(n[f], 0, T))):
            i = int(track_id[j, f])
            if i >= 0:
                first[0, i] = f if first[0, i] < 0 else first[0, i]
                last[0, i] = f
    return np.array([int(track_id.max()) + 1 if track_id.size else 0], np.int32), first, last


def features(case):
    """what the tracker's answer on the case holds, over all sequences"""
    T, S, F, ma = case["T"], case["S"], case["F"], case["max_age"]
    have = set()
    for s in range(S):
        nt, first, last = int(case["num_tracks"][s]), case["track_first"][s], case["track_last"][s]
        if (case["track_gaps"][s, :nt] > 0).any():
            have.add("coasts_and_returns")
        if (last[:nt] + ma + 1 < F).any():
            have.add("retired")
    return have


@functools.lru_cache(maxsize=None)
def stream_case(T, A, S, F_total, max_age):
    """the crafted rows of (T, A, S, F_total) at the first seed whose tracker answer holds FEATURES (born_last and row_reused depend on
    the chunking and the smoother's table: test_trajectory_stream_host.py asserts them on the stream reference)"""
    want = set(FEATURES[(T, A, S, F_total, max_age)]) - {"born_last", "row_reused"}
    for seed in range(40):
        if T == 32:
            case, ref = full_table_case("greedy", F_total, A)
        else:
            case, ref = one_shot(T, A, S, F_total, "greedy", seed=100 + seed, max_age=max_age)
        case = dict(case, max_age=max_age, **{k: ref[k] for k in ("track_id", "num_tracks", "track_first", "track_last", "track_gaps")})
        if want <= features(case):
            break
    else:
        raise AssertionError("no crafted case with %s" % sorted(want))
    rng = np.random.default_rng(seed)
    R = S * F_total
    where = rng.uniform(-0.9, 0.9, (T, R, 4)).astype(np.float32)
    where[..., 0::2] = np.abs(where[..., 0::2]) * 0.4 + 0.05
    # objects drift: a where row follows its id, so the filter has a rate to find
    for r in range(R):
        for j in range(T):
            i = int(case["track_id"][j, r])
            if i >= 0:
                where[j, r, 1::2] = np.float32(-0.5 + 0.07 * (i % 13)) + np.float32(0.04) * np.float32(r % F_total) + where[j, r, 1::2] * np.float32(0.01)
    case.update(where=where, glimpse=rng.uniform(size=(T, R, G)).astype(np.float32), G=G, img=IMG, R=R)
    s_first = prefix_tracks(case["track_id"][:, :F_total], case["n"][:F_total], T)
    nt = int(case["num_tracks"][0])
    assert s_first[0][0] <= nt and np.array_equal(s_first[1][0, :nt], case["track_first"][0, :nt])
    assert np.array_equal(s_first[2][0, :nt], case["track_last"][0, :nt])      # the ids alone give the tracker's first / last
    return case


@functools.lru_cache(maxsize=None)
def _prefix_reference(key, s, n_frames, horizon):
    case = stream_case(*key)
    T, Ft = case["T"], case["F"]
    src = slice(s * Ft, s * Ft + n_frames)
    nt, first, last = prefix_tracks(case["track_id"][:, src], case["n"][src], T)
    return trajectory.reference_smooth(case["where"][:, src], case["n"][src], case["track_id"][:, src], nt, first, last, n_frames,
                                       case["max_age"], IMG, horizon, what=case["what"][:, src], glimpse=case["glimpse"][:, src],
                                       score=case["score"][:, src], **NOISE)


def prefix_reference(key, s, n_frames, horizon=0):
    """trajectory.reference_smooth on the first n_frames frames of sequence s alone (global frame indices); shared, never modified"""
    return _prefix_reference(tuple(key), int(s), int(n_frames), int(horizon))


def cut(case, F, valids, pad="nan"):
    """the chunks of a stream over a case: per chunk the arrays the stream smoother reads at R = S F rows, sequence s holding its next
    valid[s] frames and behind them padding: NaN rows, ids and counts of 99 ("nan"), or zeros"""
    T, A, S, Ft = case["T"], case["A"], case["S"], case["F"]
    at, chunks = np.zeros(S, np.int64), []
    for v in valids:
        R = S * F
        shapes = dict(where=(T, R, 4), what=(T, R, A), glimpse=(T, R, case["G"]), score=(T, R))
        c = {k: np.full(shp, np.nan if pad == "nan" else 0.0, np.float32) for k, shp in shapes.items()}
        c["n"], c["track_id"] = np.full(R, 99 if pad == "nan" else 0, np.int32), np.full((T, R), 99 if pad == "nan" else -1, np.int32)
        for s in range(S):
            src, dst = slice(s * Ft + at[s], s * Ft + at[s] + v[s]), slice(s * F, s * F + v[s])
            for k in ("where", "what", "glimpse", "score", "track_id"):
                c[k][:, dst] = case[k][:, src]
            c["n"][dst] = case["n"][src]
        c.update(valid=np.asarray(v, np.int64), seen_before=at.copy(), T=T, A=A, S=S, F=F, G=case["G"], max_age=case["max_age"])
        chunks.append(c)
        at = at + v
    return chunks


def push(state, c, lag, horizon=0, img=IMG):
    return trajectory.reference_smooth_stream(state, c["where"], c["n"], c["track_id"], c["F"], c["valid"], lag, c["max_age"], img,
                                              horizon, what=c["what"], glimpse=c["glimpse"], score=c["score"], **NOISE)


def columns_equal(got, pre, col, ref, ref_pre, ref_col, keys=TABLE + ROWS):
    """column `col` of table `pre` in `got` against column `ref_col` of table `ref_pre` in `ref`, every key by bytes"""
    for k in keys:
        assert same(got[pre + k][:, col], ref[ref_pre + k][:, ref_col]), (pre + k, col, ref_col)
    n = int(got[pre + "count"][col])
    assert n == int(ref[ref_pre + "count"][ref_col])
    return n
