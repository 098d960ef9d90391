"""CPU tests of the stream smoother's rule (attend_infer_repeat_amd/trajectory.py: reference_smooth_stream, reference_smooth_tail and the
state helpers): fixed-lag smoothing is the one-shot rule on a truncated sequence, bit for bit, whatever the chunking.

Every comparison is by bytes: the rule is float64 + - * / in one stated order."""
import numpy as np
import pytest

from track_stream_cases import chunkings, same
from trajectory_stream_cases import (FEATURES, HOST_PARAMS, IMG, NOISE, ROWS, TABLE, columns_equal, cut, prefix_reference, push,
                                     stream_case)

from attend_infer_repeat_amd import track, trajectory
from attend_infer_repeat_amd.trajectory import ABSENT, FILLED, FORECAST, OBSERVED

HZ = 3


def lags(max_age):
    return sorted({max_age, max_age + 1, 4})


def run_stream(key, F, valids, lag, horizon=HZ, check=True):
    """the stream reference over a chunking; with check, every emitted frame, every forecast and every tail against the one-shot
    reference on the prefix.  Returns per sequence {global frame: column bytes}, the states after each chunk, what the stream held"""
    case = stream_case(*key)
    S, ma = case["S"], case["max_age"]
    chunks = cut(case, F, valids)
    state, states, emitted, held = None, [], [dict() for _ in range(S)], set()
    rows_of = [dict() for _ in range(S)]                           # table row -> ids it held
    for c in chunks:
        out, state = push(state, c, lag, horizon)
        states.append(state)
        for s in range(S):
            a, v = int(c["seen_before"][s]), int(c["valid"][s])
            b = a + v
            assert int(state["seq"][s, 0]) == b and int(state["seq"][s, 1]) == max(0, b - lag)
            want = list(range(max(0, a - lag), max(0, b - lag)))
            ne = int(out["num_emitted"][s])
            assert out["emit_frame"][s, :ne].tolist() == want and (out["emit_frame"][s, ne:] == -1).all() and ne <= v
            for e in range(ne, F):                                 # columns that emit nothing: ABSENT, count 0
                col = s * F + e
                assert out["sm_count"][col] == 0 and (out["sm_state"][:, col] == ABSENT).all() and (out["sm_id"][:, col] == -1).all()
            n_rows = 0
            for e, g in enumerate(want):
                col = s * F + e
                assert g not in emitted[s]                         # once
                emitted[s][g] = {k: out["sm_" + k][:, col].copy() for k in TABLE + ROWS + ()}
                emitted[s][g]["count"] = int(out["sm_count"][col])
                if check:
                    n_rows += columns_equal(out, "sm_", col, prefix_reference(key, s, g + lag + 1), "sm_", g)
            if check:
                C = out["sm_id"].shape[0]
                assert out["sm_counts"][s].sum() == C * ne and out["sm_counts"][s, OBSERVED] + out["sm_counts"][s, FILLED] == n_rows
                for k in range(1, horizon + 1):                    # the forecast of what has been seen
                    col = s * horizon + k - 1
                    if b == 0:
                        assert out["fc_count"][col] == 0 and (out["fc_state"][:, col] == ABSENT).all()
                    else:
                        columns_equal(out, "fc_", col, prefix_reference(key, s, b, horizon), "fc_", k - 1)
            live = {k: int(state["slots"][s, trajectory.SM_ID, k]) for k in range(32) if state["slots"][s, trajectory.SM_LIVE, k]}
            for k, i in live.items():
                rows_of[s].setdefault(k, set()).add(i)
            if v and any(int(state["slots"][s, trajectory.SM_FIRST, k]) == b - 1 for k in live):
                held.add("born_last")
        if check:
            tail = trajectory.reference_smooth_tail(state, lag, ma, IMG)
            for s in range(S):
                b = int(state["seq"][s, 0])
                want = list(range(max(0, b - lag), b))
                assert tail["tail_frame"][s, :len(want)].tolist() == want and (tail["tail_frame"][s, len(want):] == -1).all()
                for j, g in enumerate(want):
                    columns_equal(tail, "tl_", s * lag + j, prefix_reference(key, s, b), "sm_", g)
    if any(len(ids) > 1 for r in rows_of for ids in r.values()):
        held.add("row_reused")
    return emitted, states, held


@pytest.mark.parametrize("key", HOST_PARAMS, ids=lambda k: "T%d_A%d_S%d_F%d" % k[:4])
def test_truncation_identity_and_chunk_invariance(key):
    """1 and 2: each emitted frame g is column g of reference_smooth on the first g + L + 1 frames (all sm_ fields, the filled rows,
    a global src_frame), the forecast after each chunk is reference_smooth's on the first b frames, the tail its last columns; and
    the assembled emitted tables of all chunkings are byte-equal"""
    T, A, S, Ft, ma = key
    case = stream_case(*key)
    from trajectory_stream_cases import features
    held_all = features(case)
    for lag in lags(ma):
        base = None
        for name, F, valids in chunkings(S, Ft):
            emitted, _, held = run_stream(key, F, valids, lag)
            held_all |= held
            for s in range(S):
                assert sorted(emitted[s]) == list(range(max(0, Ft - lag)))
            if base is None:
                base = emitted
            else:
                for s in range(S):
                    for g, col in emitted[s].items():
                        assert all(same(col[k], base[s][g][k]) for k in TABLE + ROWS) and col["count"] == base[s][g]["count"], (name, s, g)
    assert set(FEATURES[key]) <= held_all, (FEATURES[key], held_all)


def test_a_lag_of_the_whole_video_emits_nothing_and_the_tail_is_the_one_shot_table():
    key = (3, 5, 3, 6, 1)
    case = stream_case(*key)
    S, Ft, lag = case["S"], case["F"], 6
    for name, F, valids in chunkings(S, Ft):
        state = None
        for c in cut(case, F, valids):
            out, state = push(state, c, lag)
            assert (out["num_emitted"] == 0).all() and (out["sm_state"] == ABSENT).all() and (out["emit_frame"] == -1).all()
        tail = trajectory.reference_smooth_tail(state, lag, case["max_age"], IMG)
        for s in range(S):
            assert tail["tail_frame"][s].tolist() == list(range(Ft))
            for g in range(Ft):
                columns_equal(tail, "tl_", s * lag + g, prefix_reference(key, s, Ft), "sm_", g)


def states_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert same(a[k], b[k]), k


def test_state_round_trip_pack_and_reset():
    key = (6, 50, 2, 15, 2)
    case = stream_case(*key)
    name, F, valids = chunkings(case["S"], case["F"])[4]
    chunks = cut(case, F, valids)
    lag = 3
    state, outs, states = None, [], []
    for c in chunks:
        out, state = push(state, c, lag, HZ)
        outs.append(out)
        states.append(state)
    resumed = {k: v.copy() for k, v in states[1].items()}
    kept = {k: v.copy() for k, v in resumed.items()}
    for c, out, st in zip(chunks[2:], outs[2:], states[2:]):
        o2, resumed2 = push(resumed, c, lag, HZ)
        states_equal(resumed, kept)                                # a push does not modify the state it is given
        for k in out:
            assert same(out[k], o2[k]), k
        states_equal(resumed2, st)
        resumed, kept = resumed2, {k: v.copy() for k, v in resumed2.items()}
    S, D = state["ring"].shape[:2]
    layout, size = trajectory.smooth_state_layout(S, D)
    packed = trajectory.pack_smooth_state(state)
    assert packed.dtype == np.uint8 and packed.size == size == 8 * S + 4 * S * 6 * 32 + 4 * S * D * 4 * 32 + 8 * S * D * 28 * 32
    assert all(at % 8 == 0 for at, _, _ in layout.values())
    back = trajectory.unpack_smooth_state(packed, S, D)
    for k in trajectory.SMOOTH_STATE_KEYS:
        assert same(back[k], state[k])
    before = {k: v.copy() for k, v in state.items()}
    trajectory.reset_smooth_state(state, [1])
    fresh = trajectory.new_smooth_state(S, F, lag, case["max_age"], case["T"], case["A"], case["G"])
    assert D == trajectory.ring_depth(F, lag, case["max_age"]) == F + lag + case["max_age"]
    for k in state:
        assert same(state[k][0], before[k][0]) and same(state[k][1], fresh[k][1]), k
    with pytest.raises(ValueError):
        trajectory.reset_smooth_state(state, [2])


def planted(values, seen, T=2):
    """one sequence, one track of id 0 in slot 1 (slot 0 carries no id), sighted where `seen`"""
    F = len(seen)
    where, ids = np.zeros((T, F, 4), np.float32), np.full((T, F), -1, np.int32)
    for f in range(F):
        if seen[f]:
            where[1, f], ids[1, f] = values[f], 0
    return where, np.full(F, 2, np.int32), ids


def test_the_two_exact_consequences_through_the_stream():
    """5: a one-sighting track returns its where bits; a constant track returns its value with v = 0 -- emitted, tail and forecast"""
    z = np.array([0.31, -0.47, 0.123, 0.77], np.float32)
    where, n, ids = planted([z] * 4, [1, 0, 0, 0])                 # one sighting, then retired (max_age = 1)
    state = None
    for f in range(4):
        out, state = trajectory.reference_smooth_stream(state, where[:, f:f + 1], n[f:f + 1], ids[:, f:f + 1], 1, None, 1, 1, IMG, 2)
        if f == 1:
            assert out["emit_frame"][0, 0] == 0 and out["sm_count"][0] == 1 and same(out["sm_where"][0, 0], z)
            assert out["sm_state"][0, 0] == OBSERVED and (out["sm_velocity"][0, 0] == 0).all()
            assert same(out["fc_where"][0, 0], z) and out["fc_state"][0, 1] == FORECAST      # still live: coasting
        if f >= 2:
            assert out["sm_count"][0] == 0 and (out["fc_count"] == 0).all()      # it spans frame 0 only, and is retired
    where, n, ids = planted([z] * 6, [1, 1, 0, 1, 1, 1])
    state, got = None, {}
    for f0 in (0, 2, 4):
        out, state = trajectory.reference_smooth_stream(state, where[:, f0:f0 + 2], n[f0:f0 + 2], ids[:, f0:f0 + 2], 2, None, 2, 1, IMG, 3)
        for e in range(int(out["num_emitted"][0])):
            got[int(out["emit_frame"][0, e])] = (out["sm_where"][0, e].copy(), out["sm_velocity"][0, e].copy(), int(out["sm_state"][0, e]))
        assert all(same(out["fc_where"][0, k], z) for k in range(3)) and (out["fc_velocity"] == 0).all()
    tail = trajectory.reference_smooth_tail(state, 2, 1, IMG, fill=False)
    for j in range(2):
        got[int(tail["tail_frame"][0, j])] = (tail["tl_where"][0, j].copy(), tail["tl_velocity"][0, j].copy(), int(tail["tl_state"][0, j]))
    assert sorted(got) == list(range(6))
    for g, (w, vel, st) in got.items():
        assert same(w, z) and (vel == 0).all() and st == (FILLED if g == 2 else OBSERVED)


def test_argument_refusals():
    where, n, ids = planted([np.zeros(4, np.float32)] * 2, [1, 1])
    call = lambda state=None, valid=None, lag=1, max_age=1, horizon=0: trajectory.reference_smooth_stream(
        state, where, n, ids, 2, valid, lag, max_age, IMG, horizon)
    out, state = call()
    for kw in (dict(lag=0), dict(lag=1, max_age=2), dict(lag=17), dict(lag=1.5), dict(lag=True), dict(horizon=17), dict(horizon=-1),
               dict(horizon=0.5), dict(valid=[1, 1]), dict(valid=np.array([1.0])), dict(valid=np.array([[1]]))):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(lag=0, max_age=2), dict(lag=17, max_age=1), dict(lag=1, max_age=1, horizon=17),
               # outside the supported noise domain, as air_track_smooth_stream refuses it
               dict(velocity_var=1e6), dict(velocity_var=401.0), dict(process_noise=(4.1e11, 1e-4)), dict(process_noise=(1e-4, 1e-33)),
               dict(process_noise=(1.0, 1.0), measurement_noise=3e-17, velocity_var=0.0),
               dict(process_noise=(1e-300,) * 2, measurement_noise=1e-300, velocity_var=0.0),
               dict(process_noise=(1e140,) * 2, measurement_noise=1e140)):
        with pytest.raises(ValueError):
            trajectory.check_stream_arguments(3, 4, 8, **kw)
    assert trajectory.check_stream_arguments(3, 4, 8, max_age=1, lag=16, horizon=16)[:7] == (3, 4, 2, 6, 16, 16, 21)
    assert trajectory.check_stream_arguments(3, 4, 8, max_age=2)[4] == 2 and trajectory.MAX_LAG == 16
    full = {k: v.copy() for k, v in state.items()}
    full["seq"][0] = (track.MAX_FRAMES_SEEN - 1, track.MAX_FRAMES_SEEN - 2)      # (lag 1: everything before is emitted)
    with pytest.raises(ValueError, match="int32"):
        call(full)
    call(full, valid=np.array([0]))                                # nothing fed: nothing overflows
    for k, shape in (("ring", (1, 4, 28, 31)), ("slots", (1, 8, 32)), ("seq", (2, 2)), ("what", (1, 4, 3, 1))):
        bad = {kk: v.copy() for kk, v in state.items()}
        bad[k] = np.zeros(shape, state[k].dtype)
        with pytest.raises(ValueError, match=k):
            call(bad)
    other_what = trajectory.new_smooth_state(1, 2, 1, 1, 2, 7, 1)
    with pytest.raises(ValueError, match="what rows"):
        trajectory.reference_smooth_stream(other_what, where, n, ids, 2, None, 1, 1, IMG, what=np.zeros((2, 2, 5), np.float32),
                                           glimpse=np.zeros((2, 2, 1), np.float32), score=np.zeros((2, 2), np.float32))


@pytest.mark.parametrize("max_age", [0, 1, 2])
def test_the_ring_depth_is_enough_and_one_less_is_not(max_age):
    """7: D = F + L + max_age.  One track sighted in every frame but the max_age before the first emitted frame of the third push and
    that frame itself: its FILLED row there has its source max_age frames further back, F + L + max_age - 1 frames before the newest
    frame written.  At depth D - 1 the reference's bookkeeping asserts, at D it does not"""
    F, L = 3, 2
    D = trajectory.ring_depth(F, L, max_age)
    assert D == F + L + max_age
    total = 3 * F
    g = 2 * F - L                                                  # the first frame the third push emits
    seen = [0 if (g - max_age < f <= g and max_age) else 1 for f in range(total)]
    z = [np.array([0.2, 0.01 * f, 0.2, -0.02 * f], np.float32) for f in range(total)]
    where, n, ids = planted(z, seen)
    rows = dict(what=np.arange(2 * total * 3, dtype=np.float32).reshape(2, total, 3), glimpse=np.ones((2, total, 1), np.float32),
                score=np.ones((2, total), np.float32))

    def stream(depth):
        state = trajectory.new_smooth_state(1, F, L, max_age, 2, 3, 1, depth=depth)
        outs = []
        for f0 in range(0, total, F):
            c = slice(f0, f0 + F)
            out, state = trajectory.reference_smooth_stream(state, where[:, c], n[c], ids[:, c], F, None, L, max_age, IMG, 0,
                                                            **{k: v[:, c] for k, v in rows.items()})
            outs.append(out)
        return outs

    outs = stream(D)
    assert outs[2]["emit_frame"][0, 0] == g and outs[2]["sm_state"][0, 0] == (FILLED if max_age else OBSERVED)
    assert outs[2]["sm_src_frame"][0, 0] == g - max_age and same(outs[2]["sm_what"][0, 0], rows["what"][1, g - max_age])
    stream(D + 1)
    with pytest.raises(AssertionError, match="too shallow"):
        stream(D - 1)
