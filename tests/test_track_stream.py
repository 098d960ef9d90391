"""GPU tests of stream tracking (attend_infer_repeat_amd/track.py, csrc/track_kernels.hip): air_track_associate_stream pushed chunk by
chunk against track.reference_associate_stream (every output, every tail, the state after the last chunk), the stream against the
one-shot kernels device against device, air_track_score_stream against the host and bitwise against air_track_score on the
concatenation, the argument checks, then StreamTracker end to end and the model's surface.

Bars.  Everything is compared exactly, `affinity`, the state's boxes and `what` rows by bits; the inputs are crafted rows whose one-shot
decisions are MARGIN from flipping (track_stream_cases.py says why that carries over to every chunking).  seq_iou against numpy: the
1e-12 relative of test_track.py (a sum of float64 IoUs in one stated order); device stream against device one-shot: the same bits."""
import json
import os

import numpy as np
import pytest
import torch

from test_parse import _mnist_air, _train_state, e2e_case, make_parser
from test_track import MARGIN, dev_t, frames_for, host_rows, owner_reference, run_associate, run_score, sentinel
from test_track_host import crafted_rows, moving_gt
from test_track_optimal import run_optimal
from track_stream_cases import (ROWS, assemble, check_against_one_shot, check_written, cut, full_table_case, one_shot,
                                reference_stream, same, states_equal)

from attend_infer_repeat_amd import track

pytestmark = pytest.mark.gpu

STREAM_DTYPES = dict(track_id=torch.int32, obj_state=torch.int8, affinity=torch.float32, prev_frame=torch.int32, prev_slot=torch.int32,
                     state_counts=torch.int32, num_retired=torch.int32, **{k: torch.int32 for k in track.RETIRED})
STATE_ORDER = ("st_seq", "st_slots", "st_box", "st_what")


def device_state(S, A, host=None):
    """a fresh (or given) association state as device tensors"""
    host = track.new_stream_state(S, A) if host is None else host
    return {k: dev_t(host[k]) for k in track.STATE_KEYS}


def host_state(state):
    return {k: v.cpu().numpy() for k, v in state.items()}


# ---- 1. air_track_associate_stream ----------------------------------------------------------------------------------------------------
def run_stream(chunk, state, matching, **kw):
    """air_track_associate_stream alone on one chunk (current stream), the state read and written in place; every output and a tail
    behind it start as a sentinel fill"""
    from attend_infer_repeat_amd import hip as Hh
    T, A, S, F = chunk["T"], chunk["A"], chunk["S"], chunk["F"]
    R, cap = S * F, 32 + F * T
    shapes = dict(track_id=(T, R), obj_state=(T, R), affinity=(T, R), prev_frame=(T, R), prev_slot=(T, R), state_counts=(S, 6),
                  num_retired=(S,), **{k: (S, cap) for k in track.RETIRED})
    bufs = {k: sentinel(shapes[k], STREAM_DTYPES[k]) for k in track.STREAM_OUTPUTS}
    d = {k: dev_t(chunk[k]) for k in ("what", "boxes", "score")}
    d["n"], d["valid"] = dev_t(chunk["n"].astype(np.int32)), dev_t(chunk["valid"].astype(np.int32))
    p = Hh._p
    assoc = dict(track.DEFAULTS)
    assoc.update(chunk.get("kw", {}))
    a = dict(what=p(d["what"]), boxes=p(d["boxes"]), score=p(d["score"]), n=p(d["n"]), valid=p(d["valid"]), T=T, S=S, F=F, R=R, A=A,
             matching=track.MATCHINGS.index(matching) if isinstance(matching, str) else matching, **assoc)
    a.update({"st_" + k: p(state[k]) for k in track.STATE_KEYS})
    a.update({k: p(bufs[k][0]) for k in track.STREAM_OUTPUTS})
    a.update(kw)
    st = Hh.lib().air_track_associate_stream(a["what"], a["boxes"], a["score"], a["n"], a["T"], a["S"], a["F"], a["R"], a["A"],
                                             float(a["iou_gate"]), float(a["appearance_weight"]), float(a["birth_score"]),
                                             int(a["max_age"]), a["valid"], int(a["matching"]), *[a[k] for k in STATE_ORDER],
                                             *[a[k] for k in track.STREAM_OUTPUTS], Hh._stream())
    torch.cuda.synchronize()
    got, tails = {}, {}
    for k in track.STREAM_OUTPUTS:
        n = int(np.prod(shapes[k]))
        got[k], tails[k] = bufs[k][0][:n].view(shapes[k]).cpu().numpy(), bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, tails, {k: bufs[k][1] for k in track.STREAM_OUTPUTS}


def stream_case(name, matching):
    """(one-shot case, chunk_frames, [valid per chunk]) of the five shapes (T, A, S, F_chunk, chunks)"""
    even = lambda S, F, n: [np.full(S, F, np.int64)] * n
    if name == "1,1,1,1,3":
        return one_shot(1, 1, 1, 3, matching)[0], 1, even(1, 1, 3)
    if name == "3,5,3,2,3 ragged":
        return one_shot(3, 5, 3, 6, matching)[0], 2, [np.array(v, np.int64) for v in ([2, 1, 0], [0, 2, 2], [2, 2, 1])]
    if name == "6,50,2,5,3":
        return one_shot(6, 50, 2, 15, matching, iou_gate=0.2, appearance_weight=0.6, birth_score=0.4, max_age=2)[0], 5, even(2, 5, 3)
    if name == "32,5,1,2,3 full table":
        return full_table_case(matching)[0], 2, even(1, 2, 3)
    return one_shot(3, 50, 1, 6, matching)[0], 1, even(1, 1, 6)


@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("name", ["1,1,1,1,3", "3,5,3,2,3 ragged", "6,50,2,5,3", "32,5,1,2,3 full table", "3,50,1,1,6"])
def test_associate_stream_is_the_reference(gpu_device, name, matching):
    case, F, valids = stream_case(name, matching)
    chunks = cut(case, F, valids, pad="nan")
    want, want_states = reference_stream(chunks, matching)
    state, outs = device_state(case["S"], case["A"]), []
    for c, (chunk, ref) in enumerate(zip(chunks, want)):
        st, got, tails, fill = run_stream(chunk, state, matching)
        assert st == 0
        for k in track.STREAM_OUTPUTS:                             # every element: the reference defines all of them, none is the fill
            assert tails[k], (k, c)
            assert same(got[k], ref[k]), (k, c, got[k], ref[k])
            assert not (ref[k] == fill[k]).any(), k
        check_written(got, chunk)
        states_equal(host_state(state), want_states[c])
        outs.append(got)
    fed = np.sum(valids, 0)
    check_against_one_shot(assemble(outs, chunks), host_state(state), case, matching, fed)
    if "full table" in name:
        assert all(s["slots"][0, track.ST_LIVE].all() for s in want_states)      # all 32 slots live across both boundaries
    print("tracks", host_state(state)["seq"][:, 1].tolist(), "retired", [o["num_retired"].tolist() for o in outs])


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_stream_is_the_one_shot_kernel_device_against_device(gpu_device, matching):
    for case in (one_shot(3, 5, 3, 6, matching)[0], one_shot(6, 50, 2, 6, matching, max_age=2)[0], full_table_case(matching)[0]):
        st, whole, tails, _ = (run_optimal if matching == "optimal" else run_associate)(case)
        assert st == 0 and all(tails.values())
        S, Ft, F = case["S"], case["F"], 2
        chunks = cut(case, F, [np.full(S, F, np.int64)] * (Ft // F))
        state, outs = device_state(S, case["A"]), []
        for chunk in chunks:
            st, got, tails, _ = run_stream(chunk, state, matching)
            assert st == 0 and all(tails.values())
            outs.append(got)
        for s, per in enumerate(assemble(outs, chunks)):
            for k in ROWS:                                         # (prev_frame: the stream gives the global index, which is the
                want = whole[k][:, s * Ft:(s + 1) * Ft]            #  one-shot kernel's on a sequence walked from its frame 0)
                assert same(per["rows"][k], want), (k, s)
            assert np.array_equal(per["counts"], whole["state_counts"][s])
        assert host_state(state)["seq"][:, 1].tolist() == whole["num_tracks"].tolist()


def test_associate_stream_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, _ = one_shot(3, 5, 2, 4, "greedy", seed=8)
    chunk = cut(case, 4, [np.full(2, 4, np.int64)])[0]
    off = torch.zeros(2 * 32 * 4 + 1, device="cuda")
    start = track.new_stream_state(2, 5)
    start["seq"][:] = 7                                            # a state that a run would change
    for kw, code in ((dict(what=None), -1), (dict(n=None), -1), (dict(valid=None), -1), (dict(st_seq=None), -1), (dict(st_slots=None), -1),
                     (dict(st_box=None), -1), (dict(st_what=None), -1), (dict(track_id=None), -1), (dict(num_retired=None), -1),
                     (dict(retired_gaps=None), -1), (dict(matching=2), -2), (dict(matching=-1), -2), (dict(T=0), -2), (dict(T=33), -2),
                     (dict(R=9), -2), (dict(iou_gate=1.0), -2), (dict(max_age=-1), -2), (dict(boxes=Hh._p(off[1:])), -3),
                     (dict(st_box=Hh._p(off[1:])), -3)):
        state = device_state(2, 5, start)
        kw = dict(kw)
        st, got, tails, fill = run_stream(chunk, state, kw.pop("matching", "greedy"), **kw)
        assert st == code, kw
        assert all(tails.values()) and all((got[k] == fill[k]).all() for k in track.STREAM_OUTPUTS), kw
        states_equal(host_state(state), start)
    big = dict(what=np.zeros((32, 1, 1), np.float32), boxes=np.zeros((32, 1, 4), np.float32), score=np.zeros((32, 1), np.float32),
               n=np.zeros(1, np.int32), valid=np.ones(1, np.int64), T=32, A=1, S=1, F=1)
    state = device_state(1, 1)
    st, got, tails, fill = run_stream(big, state, "greedy", F=1024, S=1, R=1024)      # 1024 * 32 > 32767 (nothing is read: refused first)
    assert st == -2 and all((got[k] == fill[k]).all() for k in track.STREAM_OUTPUTS)
    states_equal(host_state(state), track.new_stream_state(1, 1))


# ---- 2. air_track_score_stream -----------------------------------------------------------------------------------------------------------
def run_score_stream(chunk, ids_host, gt_host, state, tau=0.5, **kw):
    from attend_infer_repeat_amd import hip as Hh
    T, S, F = chunk["T"], chunk["S"], chunk["F"]
    R, G = S * F, gt_host.shape[1]
    shapes = dict(seq_counts=((S, 8), torch.int32), seq_iou=((S,), torch.float64), gt_match=((R, G), torch.int32))
    bufs = {k: sentinel(*v) for k, v in shapes.items()}
    d = dict(boxes=dev_t(chunk["boxes"]), n=dev_t(chunk["n"].astype(np.int32)), ids=dev_t(ids_host.astype(np.int32)), gt=dev_t(gt_host),
             valid=dev_t(chunk["valid"].astype(np.int32)))
    p = Hh._p
    a = dict(boxes=p(d["boxes"]), n=p(d["n"]), ids=p(d["ids"]), gt=p(d["gt"]), valid=p(d["valid"]), tau=tau, T=T, G=G, S=S, F=F, R=R,
             score_i=p(state["score_i"]), score_f=p(state["score_f"]))
    a.update({k: p(bufs[k][0]) for k in shapes})
    a.update(kw)
    st = Hh.lib().air_track_score_stream(a["boxes"], a["n"], a["ids"], a["gt"], float(a["tau"]), a["T"], a["G"], a["S"], a["F"], a["R"],
                                         a["valid"], a["score_i"], a["score_f"], a["seq_counts"], a["seq_iou"], a["gt_match"],
                                         Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, (shape, _) in shapes.items():
        n = int(np.prod(shape))
        got[k] = bufs[k][0][:n].view(shape).cpu().numpy()
        clean = clean and bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, clean, {k: bufs[k][1] for k in shapes}


def cut_score(case, ids, gt, F, valids):
    """the chunks of cut() with the ids and the ground truth cut alongside (padding: ids of 77, boxes of ones)"""
    S, Ft, T, G = case["S"], case["F"], case["T"], gt.shape[1]
    chunks, at = cut(case, F, valids, pad="nan"), np.zeros(S, np.int64)
    for chunk, v in zip(chunks, valids):
        tid, g = np.full((T, S * F), 77, np.int32), np.ones((S * F, G, 4), np.float32)
        for s in range(S):
            src, dst = slice(s * Ft + at[s], s * Ft + at[s] + v[s]), slice(s * F, s * F + v[s])
            tid[:, dst], g[dst] = ids[:, src], gt[src]
        chunk["ids"], chunk["gt"] = tid, g
        at = at + v
    return chunks


@pytest.mark.parametrize("T,S,F_total,G,tau,F,valids", [
    (3, 3, 6, 8, 0.5, 2, ([2, 1, 0], [0, 2, 2], [2, 2, 2], [2, 1, 2])), (6, 2, 15, 8, 0.3, 5, ([5, 5], [5, 5], [5, 5])),
    (32, 1, 6, 8, 0.5, 1, ([1],) * 6), (1, 3, 2, 1, 0.0, 2, ([2, 2, 2],))])
def test_score_stream_is_the_reference_and_the_one_shot_bits(gpu_device, T, S, F_total, G, tau, F, valids):
    case, ref = crafted_rows(T, 5, S, F_total, seed=T + S + F_total + G)
    rng = np.random.default_rng(T + G)
    gt = moving_gt(case, rng, G)
    ids = ref["track_id"].copy()
    flip = rng.uniform(size=ids.shape) < 0.1
    ids[flip & (ids >= 0)] += 1
    valids = [np.array(v, np.int64) for v in valids]
    assert (np.sum(valids, 0) == F_total).all()
    st, whole, clean, _ = run_score(case, ids, gt, tau)
    assert st == 0 and clean
    host = track.new_score_state(S)
    state = {k: dev_t(host[k]) for k in track.SCORE_STATE_KEYS}
    want_state, matches = None, [[] for _ in range(S)]
    for chunk in cut_score(case, ids, gt, F, valids):
        want, want_state = track.reference_score_stream(want_state, chunk["boxes"], chunk["n"], chunk["ids"], chunk["gt"], F,
                                                        chunk["valid"], tau)
        st, got, clean, _ = run_score_stream(chunk, chunk["ids"], chunk["gt"], state, tau)
        assert st == 0 and clean
        assert np.array_equal(got["seq_counts"], want["seq_counts"]) and np.array_equal(got["gt_match"], want["gt_match"])
        assert np.all(np.abs(got["seq_iou"] - want["seq_iou"]) <= 1e-12 * np.abs(want["seq_iou"]))
        assert np.array_equal(state["score_i"].cpu().numpy(), want_state["score_i"])
        for s in range(S):
            matches[s].append(got["gt_match"][s * F:s * F + int(chunk["valid"][s])])
    assert np.array_equal(got["seq_counts"], whole["seq_counts"])
    assert np.array_equal(got["seq_iou"].view(np.uint64), whole["seq_iou"].view(np.uint64))      # continued: the one-shot kernel's bits
    assert np.array_equal(state["score_f"].cpu().numpy().view(np.uint64), whole["seq_iou"].view(np.uint64))
    assert np.array_equal(np.concatenate([np.concatenate(m) for m in matches]), whole["gt_match"])
    assert whole["seq_counts"][:, 0].sum() > 0


def test_score_stream_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, ref = crafted_rows(3, 5, 2, 4, seed=8)
    gt = moving_gt(case, np.random.default_rng(0), 2)
    chunk = cut_score(case, ref["track_id"], gt, 4, [np.full(2, 4, np.int64)])[0]
    off = torch.zeros(2 * 8 * 4 + 1, device="cuda")
    start = track.new_score_state(2)
    start["score_i"][:, :5] = 3
    for kw, code in ((dict(boxes=None), -1), (dict(valid=None), -1), (dict(score_i=None), -1), (dict(score_f=None), -1),
                     (dict(seq_iou=None), -1), (dict(T=0), -2), (dict(G=9), -2), (dict(R=9), -2), (dict(tau=1.5), -2),
                     (dict(gt=Hh._p(off[1:])), -3)):
        state = {k: dev_t(start[k]) for k in track.SCORE_STATE_KEYS}
        st, got, clean, fill = run_score_stream(chunk, chunk["ids"], chunk["gt"], state, **kw)
        assert st == code, kw
        assert clean and all((got[k] == fill[k]).all() for k in got), kw
        assert np.array_equal(state["score_i"].cpu().numpy(), start["score_i"]) and (state["score_f"].cpu().numpy() == 0).all()


# ---- 3. StreamTracker ---------------------------------------------------------------------------------------------------------------------
def make_stream(name, S, F, capture=False, **kw):
    from attend_infer_repeat_amd.track import StreamTracker
    ocfg, _, params, _ = e2e_case(name)
    ps = make_parser(ocfg, S * F, params)
    tk = StreamTracker(ps, F, **kw)
    if capture:
        ps.capture()
        tk.capture()
    return ocfg, tk, ps


KEYS = ROWS + ("state_counts", "num_retired", "track_owner") + track.RETIRED
PUSHES = ([2, 2, 2], [2, 2, 2], [2, 1, 0])                         # three pushes, the last one ragged


def push_all(tk, ocfg, S, F, counts, seed=21):
    """the three pushes on frames of one moving batch; returns per push (the result cloned, the host rows of the provider)"""
    frames = frames_for(ocfg, S, F * len(PUSHES), seed=seed).cuda()
    done = []
    for c, v in enumerate(PUSHES):
        out = tk.push(frames[:, c * F:(c + 1) * F].contiguous(), np.array(v), counts[c])
        tk.synchronize()
        done.append({k: (x.clone() if torch.is_tensor(x) else x) for k, x in out.items()})
    return done


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_stream_tracker_is_provider_then_the_stream_reference(gpu_device, matching):
    S, F = 3, 2
    rule = dict(iou_gate=0.05, birth_score=0.0)                    # (an untrained model's scores are low)
    ocfg, tk, ps = make_stream("tiny", S, F, capture=True, matching=matching, **rule)
    _, eager, _ = make_stream("tiny", S, F, matching=matching, **rule)
    T, R = ocfg.max_steps, S * F
    assert (tk.T, tk.R, tk.S, tk.F) == (T, R, S, F) and tk.engine is ps.engine and tk._graph is not None and eager._graph is None
    assert tk.launch_count()["track_associate_stream"] == 1 and list(tk.segments) == ["associate", "owner"]
    rng = np.random.default_rng(9)
    counts = [torch.from_numpy(rng.integers(0, T + 1, R).astype(np.int32)).cuda() for _ in PUSHES]      # (random weights may see nothing)
    done = push_all(tk, ocfg, S, F, counts)
    assert tk.frames_seen.tolist() == [6, 5, 4] and tk.state["seq"][:, 0].tolist() == [6, 5, 4]
    state, safe = None, np.ones(S, bool)
    for c, (got, v) in enumerate(zip(done, PUSHES)):
        rows = host_rows(got, T, R)                                # the provider's own rows, read back per chunk
        want, state = track.reference_associate_stream(state, rows["what"], rows["boxes"], rows["score"], rows["n"], F, np.array(v),
                                                       matching=matching, return_margins=True, **rule)
        safe &= (want["gate_margin"] >= MARGIN) & (want.get("round_margin", want["gate_margin"]) >= MARGIN)
        in_rows = np.repeat(safe, F)
        for k in KEYS[:-6] + track.RETIRED:
            g = got[k].cpu().numpy()
            g, w = (g[:, in_rows], want[k][:, in_rows]) if k in ROWS else (g[safe], want[k][safe])
            assert same(g, w), (k, c)
        owner = got["owner"].cpu().numpy()
        assert np.array_equal(got["track_owner"].cpu().numpy(), owner_reference(owner, got["track_id"].cpu().numpy(), T))
        assert got["track_owner"].dtype == torch.int16 and set(got) >= set(KEYS)
    print("sequences inside the margins: %d of %d; ids issued %s" % (safe.sum(), S, state["seq"][:, 1].tolist()))
    assert safe.sum() >= S - 1 and state["seq"][:, 1].sum() > 0    # (a decision within rounding of flipping proves nothing either way)
    final = host_state({k: tk.state[k] for k in track.STATE_KEYS})
    for k in track.STATE_KEYS:
        assert same(final[k][safe], state[k][safe]), k
    live = tk.live()
    assert live["id"].data_ptr() == tk.state["slots"][:, track.ST_ID].data_ptr() and tuple(live["what"].shape) == (S, 32, tk.A)
    # captured equals eager, chunk by chunk
    again = push_all(eager, ocfg, S, F, counts)
    for a, b in zip(done, again):
        for k in KEYS + ("num_objects", "boxes", "owner"):
            assert torch.equal(a[k], b[k]), k
    for k in track.STATE_KEYS:
        assert torch.equal(tk.state[k], eager.state[k]), k
    tk.release_graphs()


def test_a_restored_state_repeats_the_pushes_and_the_provider_is_untouched(gpu_device):
    S, F = 3, 2
    ocfg, tk, ps = make_stream("tiny", S, F, capture=True, iou_gate=0.05, birth_score=0.0)
    T, R = ocfg.max_steps, S * F
    rng = np.random.default_rng(9)
    counts = [torch.from_numpy(rng.integers(0, T + 1, R).astype(np.int32)).cuda() for _ in PUSHES]
    frames = frames_for(ocfg, S, F * 3, seed=21).cuda()
    chunk = lambda c: frames[:, c * F:(c + 1) * F].contiguous()
    tk.push(chunk(0), None, counts[0])
    saved = tk.state_dict()
    assert set(saved) == set(track.STATE_KEYS + track.SCORE_STATE_KEYS) and saved["seq"].data_ptr() != tk.state["seq"].data_ptr()
    first = []
    for c in (1, 2):
        out = tk.push(chunk(c), np.array(PUSHES[c]), counts[c])
        tk.synchronize()
        first.append({k: out[k].clone() for k in KEYS})
    after = tk.state_dict()
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    base = ps.parse(chunk(2).reshape(R, *ocfg.img_size), counts[2])      # the provider's result is what a plain parse() gives
    ps.synchronize()
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t
    for k in base:
        assert torch.equal(raw(out[k]), raw(base[k])) if torch.is_tensor(base[k]) else out[k] == base[k], k
    assert first[0]["track_id"].max() >= 0
    # pushing on continues the stream: not idempotent ...
    moved = tk.push(chunk(2), np.array(PUSHES[2]), counts[2])
    tk.synchronize()
    assert tk.frames_seen.tolist() == [8, 6, 4] and not torch.equal(tk.state["seq"], after["seq"])
    # ... and the saved state brings the same bits back
    tk.load_state_dict(saved)
    assert tk.frames_seen.tolist() == [2, 2, 2]
    for c, want in zip((1, 2), first):
        out = tk.push(chunk(c), np.array(PUSHES[c]), counts[c])
        tk.synchronize()
        for k in KEYS:
            assert torch.equal(out[k], want[k]), (k, c)
    for k in after:
        assert torch.equal(raw(tk.state[k]), raw(after[k])), k
    # reset: one sequence alone, then all
    tk.reset([1])
    tk.synchronize()
    fresh = track.new_stream_state(S, tk.A)
    now = host_state({k: tk.state[k] for k in track.STATE_KEYS})
    for k in track.STATE_KEYS:
        assert same(now[k][1], fresh[k][1]) and same(now[k][[0, 2]], after[k].cpu().numpy()[[0, 2]]), k
    assert tk.frames_seen.tolist() == [6, 0, 4]
    tk.reset()
    states_equal(host_state({k: tk.state[k] for k in track.STATE_KEYS}), fresh)
    with pytest.raises(ValueError, match="valid"):
        tk.push(chunk(0), np.zeros(2, np.int64), counts[0])
    with pytest.raises(ValueError, match="frames"):
        tk.push(frames[:, :3], None, counts[0])
    tk.frames_seen[2] = 2 ** 31 - 2
    with pytest.raises(ValueError, match="frames_seen"):
        tk.push(chunk(0), None, counts[0])
    states_equal(host_state({k: tk.state[k] for k in track.STATE_KEYS}), fresh)       # a refused push runs nothing
    tk.release_graphs()


def test_stream_tracker_scores_across_chunks(gpu_device):
    S, F, G = 3, 2, 2
    ocfg, tk, ps = make_stream("rect_t5", S, F, capture=True, birth_score=0.0)
    T, R = ocfg.max_steps, S * F
    frames = frames_for(ocfg, S, F * 3, seed=31).cuda()
    state, want = None, None
    assert tk.summary()["gt"] == 0 and np.isnan(tk.summary()["mota"])
    for c, v in enumerate(PUSHES):
        out = tk.push(frames[:, c * F:(c + 1) * F].contiguous(), np.array(v))
        tk.synchronize()
        rows = host_rows(out, T, R)
        gt = moving_gt(dict(boxes=rows["boxes"], n=rows["n"], T=T, S=S, F=F), np.random.default_rng(c), G)
        got = tk.score(torch.from_numpy(gt.reshape(S, F, G, 4)))
        tk.synchronize()
        want, state = track.reference_score_stream(state, rows["boxes"], rows["n"], out["track_id"].cpu().numpy(), gt, F, np.array(v))
        assert np.array_equal(got["seq_counts"].cpu().numpy(), want["seq_counts"]) and np.array_equal(got["gt_match"].cpu().numpy(), want["gt_match"])
        assert np.allclose(got["seq_iou"].cpu().numpy(), want["seq_iou"], rtol=1e-12, atol=0)
    summary = tk.summary()
    mine = track.mot_summary(want["seq_counts"].sum(0), float(got["seq_iou"].sum().item()))
    assert set(summary) == set(mine) and all(summary[k] == mine[k] or (np.isnan(summary[k]) and np.isnan(mine[k])) for k in mine)
    assert summary["gt"] > 0
    with pytest.raises(ValueError, match="score_reset"):
        tk.score(torch.from_numpy(gt), tau=0.3)
    tk.score_reset()
    assert tk.summary()["gt"] == 0 and (tk.state["score_i"][:, 8:16] == -1).all() and tk.state["seq"][:, 0].tolist() == [6, 5, 4]
    tk.release_graphs()


def test_stream_refusals(gpu_device):
    import types
    from attend_infer_repeat_amd.track import StreamTracker
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 10, params)
    with pytest.raises(ValueError, match="multiple"):
        StreamTracker(ps, 3)
    with pytest.raises(ValueError, match="matching"):
        StreamTracker(ps, 5, matching="best")
    with pytest.raises(ValueError, match="ParticleParser"):
        StreamTracker(types.SimpleNamespace(KIND="particle", engine=ps.engine, R=10, T=3), 5)


# ---- 4. surface -----------------------------------------------------------------------------------------------------------------------
def test_track_stream_on_the_model_continues_ids_and_does_not_disturb_training(gpu_device):
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    B, S, F, T = 8, 2, 2, 3
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    d = procedural_moving_mnist(S, 2 * F, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    before, obs_before = _train_state(air._engine), air.obs
    rule = dict(birth_score=0.0, iou_gate=0.05)
    a = {k: v.clone() for k, v in air.track_stream(frames[:, :F], **rule).items() if torch.is_tensor(v)}
    b = air.track_stream(frames[:, F:], **rule)
    air._engine.synchronize()
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air.obs is obs_before and air._engine.global_step == 2 and air.tracked_stream is b
    tk = air.stream_tracker(S, F, **rule)
    assert tk is air.stream_tracker(S, F, **rule) and tk._graph is not None and len(air._trackers) == 1
    assert tk.frames_seen.tolist() == [4, 4] and tk.state["seq"][:, 0].tolist() == [4, 4]
    R = S * F
    assert tuple(b["track_id"].shape) == (T, R) and tuple(b["retired_id"].shape) == (S, 32 + F * T) and b["track_owner"].dtype == torch.int16
    # the second call continues the first: the host stream reference on the provider's own rows of the two calls, ids included
    state, safe = None, np.ones(S, bool)
    for got in (a, b):
        rows = host_rows(got, T, R)
        want, state = track.reference_associate_stream(state, rows["what"], rows["boxes"], rows["score"], rows["n"], F,
                                                       return_margins=True, **rule)
        safe &= (want["gate_margin"] >= MARGIN) & (want["round_margin"] >= MARGIN)
        for k in ROWS:
            assert same(got[k].cpu().numpy()[:, np.repeat(safe, F)], want[k][:, np.repeat(safe, F)]), k
    assert safe.any() and state["seq"][safe, 1].sum() > 0
    assert np.array_equal(tk.state["seq"].cpu().numpy()[safe], state["seq"][safe])
    matched = b["obj_state"] == track.MATCHED
    assert matched.any() and (b["prev_frame"][matched] >= F - 1).all()      # global frame indices: a chunk-local one would be < F
    born_b = b["track_id"][b["obj_state"] == track.BORN]
    assert (born_b >= a["track_id"].max() + 1).all()                # ids go on where the first call stopped
    air.track(frames, **rule)
    assert len(air._trackers) == 2 and air.tracker(S, 2 * F, **rule) is not tk      # a key of its own, the same bound
    again = air.track_stream(frames[:, :F], reset=True, **rule)
    assert all(torch.equal(again[k], a[k]) for k in KEYS) and tk.frames_seen.tolist() == [2, 2]
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params) and torch.equal(air._engine.rng_state, twin._engine.rng_state)
    with pytest.raises(ValueError, match="frames"):
        air.track_stream(frames[0])
    assert air.obs is obs_before


def test_training_script_track_stream_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "5:2.5",
                            "--track-stream", "2"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_stream"]
    one = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" track stream ") == 2
    for l, o in zip(rec, one):
        assert l["n_frames"] == 5 and l["chunk_frames"] == 2 and l["matching"] == "greedy"
        assert l["gt"] == o["gt"] > 0 and l["gt_objects"] == o["gt_objects"] and l["matches"] + l["misses"] == l["gt"]
        assert l["tracks"] >= 0 and (l["mota"] <= 1.0 or np.isnan(l["mota"])) and l["max_age"] == track.DEFAULTS["max_age"]
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-stream", "2"])
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-stream", "0"])
