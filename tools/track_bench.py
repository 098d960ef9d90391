#!/usr/bin/env python
"""Measurements of sequence tracking (attend_infer_repeat_amd/track.py); prints one JSON line and a readable table.

For every F in --frames (default 8 and 32) at --rows provider rows (default 1024: S = rows / F sequences of 50 x 50 frames, T = 3):
a captured SceneParser with untrained parameters and given counts r mod (T + 1), so that every frame count occurs, and a captured
SequenceTracker over it with birth_score = 0 (an untrained model's scores are low: every finite object may start a track, so the
matching loop has work).  The frames of a sequence are one sparse random image shifted a pixel per frame.

  agreement  the tracker's outputs against track.reference_associate on the read-back of the same parse: the sequences whose decisions
             are at least 1e-9 from flipping must agree exactly, or the tool exits with an error;
  provider   the provider's own captured parse() of the R rows;
  tracked    the captured track() of the same rows (provider + tail);
  tail       the tracker's own graph alone (air_track_associate + air_track_owner), replayed on the engine's stream;
  score      the air_track_score graph alone, against ground truth cut from the parse's own boxes;
  and every entry launched eagerly on its own.

--matching optimal adds a second captured tracker with matching="optimal" over the SAME parser: its agreement with
track.reference_associate(matching="optimal"), the share of frames (and sequences) on which its track ids differ from the greedy
tracker's, its tail graph timed in turns with the greedy one (greedy, optimal, greedy, optimal) in this process, and
air_track_associate_optimal launched eagerly beside air_track_associate.  --identity scores with identity=True: the air_track_score +
air_track_idf graph beside the air_track_score graph, air_track_idf eagerly beside air_track_score, and the IDF figures.

--stream CHUNK [CHUNK ...] measures stream tracking instead (track.StreamTracker): for every CHUNK, at --rows provider rows (S = rows /
CHUNK sequences), ONE captured SceneParser with a captured SequenceTracker(F = CHUNK) and a captured StreamTracker(chunk_frames = CHUNK)
over it.  --stream-chunks chunks (default 4) of one moving sequence are pushed; the stream's track ids of every chunk are compared with
track.reference_associate (the ONE-SHOT rule) on the concatenation of the provider's rows read back chunk by chunk -- the share of
(chunk, sequence) pairs that agree is printed and must be 1 over the sequences whose decisions are 1e-9 from flipping, or the tool
exits with an error -- and the first chunk of a fresh stream with the one-shot tracker's device outputs.  Then the two captured tails
(associate + owner) are timed in turns (one-shot, stream, one-shot, stream) in this process on the engine's stream, the stream restarted
before each turn, and the ratio is reported; the whole calls (`track()` and `push()`, provider included) likewise; the stream launch
alone with valid = 0; no bar on time.

--motion measures motion-predicted association instead (track.SequenceTracker(motion=True): air_track_associate_motion): for every
F in --frames, at --rows provider rows, ONE captured SceneParser and over it, for both matchings, a captured tracker without motion
(air_track_associate / air_track_associate_optimal: the kernels of the commit before, whose instantiations did not change) and one
with motion at the default noise terms.  The motion tracker's outputs, pred_where and pred_boxes included, must agree bit for bit with
track.reference_associate_motion on the read-back of the same parse over the sequences whose decisions are 1e-9 from flipping, or the
tool exits with an error; the share of frames on which motion changes a track id is printed.  Then the two captured tails (associate +
owner) are timed in turns (plain, motion, plain, motion) in this process on the engine's stream, and the ratio is reported, with the
two association entries launched eagerly on their own; no bar on time.

--motion --gate measures the Mahalanobis gate on top (track.SequenceTracker(motion=True, motion_gate=True):
air_track_associate_motion_gated) the same way, against the motion tracker WITHOUT the gate of the same build: the gated tracker must
agree bit for bit with track.reference_associate_motion(gate=True), pred_d2 included, over the sequences inside the margins; the two
captured tails are timed in turns (motion, gated, motion, gated) in this process, and the ratio is reported; no bar on time.

--hota measures the HOTA metric instead (SequenceTracker.hota: air_track_hota): for every F in --frames, at --rows provider rows, ONE
captured SceneParser and a captured tracker (--matching) over it; ground truth cut from the parse's own boxes, every fifth frame
shifted by 1.5 px so that the thresholds part.  The device outputs of the first --hota-check sequences must equal
track.reference_hota bit for bit, or the tool exits with an error.  Then the three captured graphs -- air_track_score, air_track_score
+ air_track_idf, air_track_hota -- are timed in turns in this process, and the three entries launched eagerly, in turns as well (5
repeats of --iters back-to-back launches between two device events) and one launch at a time as the other modes time it; the ratios
are reported; no bar on time.

--mots measures the MOTS measures instead (SequenceTracker.mots: the unchanged air_score_contingency, then air_track_mots): the same
tracker; the instance maps are cut from the parse's own owner map (labels below 3), every fifth frame rolled two pixels, which takes
those frames below IoU 1/2 (the misses and false positives of the figures).  cont and the four outputs of the first --mots-check
sequences must equal track.mots_contingency and track.reference_mots bit for bit, or the tool exits with an error.  Then the two
captured graphs -- air_track_score and the MOTS pair -- are timed in turns in this process, and the three entries launched eagerly,
in turns as well and one launch at a time; the ratios are reported; no bar on time.

--stitch measures stitching (track.TrackStitcher: air_track_stitch, then air_track_owner on the stitched ids): for every F in --frames, at
--rows provider rows, ONE captured SceneParser, a captured tracker (--matching, max_age 1) and a captured stitcher over it; the counts
leave two frames in five empty, so the tracks die and are born again and the stitcher has fragments to join.  The device outputs of the
first --stitch-check sequences must equal track.reference_stitch bit for bit, or the tool exits with an error.  Then the two captured
graphs -- the tracker's tail (associate + owner) and the stitcher's (stitch + owner) -- are timed in turns in this process, and the
three entries launched eagerly, in turns as well; the ratios are reported; no bar on time.  Last, the stitch launch alone with max_gap = 1
and with a gate that admits nothing: where its time goes, by difference.

Timing: a warm-up, then 5 repeats of --iters calls each between device events; the median repeat is reported with all repeats.  The
provider and the tracked route alternate inside one process."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def median_ms(fn, iters, stream):
    fn(); fn()
    torch.cuda.synchronize()
    reps = [timed(fn, iters, stream) for _ in range(5)]
    return statistics.median(reps), reps


def one_length(args, F):
    from attend_infer_repeat_amd import _lib, track
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T, G = R // F, int(cfg.max_steps), 3
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    tk = track.SequenceTracker(ps, F, birth_score=0.0)
    tk.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    stream = torch.cuda.current_stream()
    # agreement first
    out = tk.track(frames, counts)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    ref = track.reference_associate(host(out["what"]).reshape(T, R, -1), host(out["boxes"]), host(out["score"]), host(out["num_objects"]),
                                    F, birth_score=0.0, return_margins=True)
    safe = (ref["gate_margin"] >= 1e-9) & (ref["round_margin"] >= 1e-9)
    rows = np.repeat(safe, F)
    agree = {}
    for k in ("track_id", "obj_state", "prev_frame", "prev_slot"):
        agree[k] = bool((host(out[k])[:, rows] == ref[k][:, rows]).all())
    agree["affinity_bits"] = bool((host(out["affinity"])[:, rows].view(np.uint32) == ref["affinity"][:, rows].view(np.uint32)).all())
    for k in ("num_tracks", "track_first", "track_last", "track_length", "track_gaps", "state_counts"):
        agree[k] = bool((host(out[k])[safe] == ref[k][safe]).all())
    res = dict(frames=F, sequences=S, rows=R, max_steps=T, sequences_inside_margins=int(safe.sum()), agreement=agree,
               tracks=int(ref["num_tracks"].sum()), state_counts=dict(zip(track.STATES, ref["state_counts"].sum(0).tolist())))
    if not all(agree.values()):
        print(json.dumps(res))
        raise SystemExit("the tracker and the host reference disagree: %r" % (agree,))
    boxes, n = host(out["boxes"]), host(out["num_objects"])
    gt = np.zeros((R, G, 4), np.float32)
    for g in range(G):
        gt[n > g, g] = boxes[g, n > g]
    gt = torch.from_numpy(gt).to(dev)
    tk.score(gt, accumulate=False)
    res["score_summary"] = tk.summary()
    entry = next(iter(tk._score.values()))
    opt = None
    if args.matching == "optimal":
        opt = track.SequenceTracker(ps, F, birth_score=0.0, matching="optimal")
        opt.capture()
        greedy_ids = host(out["track_id"]).copy()
        oo = opt.track(frames, counts)
        torch.cuda.synchronize()
        oref = track.reference_associate(host(oo["what"]).reshape(T, R, -1), host(oo["boxes"]), host(oo["score"]), host(oo["num_objects"]),
                                         F, birth_score=0.0, return_margins=True, matching="optimal")
        osafe = oref["gate_margin"] >= 1e-9
        orows = np.repeat(osafe, F)
        oagree = {k: bool((host(oo[k])[:, orows] == oref[k][:, orows]).all()) for k in ("track_id", "obj_state", "prev_frame", "prev_slot")}
        oagree["affinity_bits"] = bool((host(oo["affinity"])[:, orows].view(np.uint32) == oref["affinity"][:, orows].view(np.uint32)).all())
        for k in ("num_tracks", "track_first", "track_last", "track_length", "track_gaps", "state_counts"):
            oagree[k] = bool((host(oo[k])[osafe] == oref[k][osafe]).all())
        differ = (host(oo["track_id"]) != greedy_ids).any(0)
        res.update(optimal_agreement=oagree, optimal_sequences_inside_margin=int(osafe.sum()), optimal_tracks=int(oref["num_tracks"].sum()),
                   optimal_state_counts=dict(zip(track.STATES, oref["state_counts"].sum(0).tolist())),
                   frames_where_matchings_differ=float(differ.mean()),
                   sequences_where_matchings_differ=float(differ.reshape(S, F).any(1).mean()))
        if not all(oagree.values()):
            print(json.dumps(res))
            raise SystemExit("the optimal tracker and the host reference disagree: %r" % (oagree,))
        opt.score(gt, accumulate=False, identity=args.identity)
        res["optimal_score_summary"] = opt.summary()
        if args.identity:
            res["optimal_identity_summary"] = opt.identity_summary()
    id_entry = None
    if args.identity:
        tk.track(frames, counts)
        tk.score(gt, accumulate=False, identity=True)
        res["identity_summary"] = tk.identity_summary()
        id_entry = tk._score[(G, 0.5, "idf")]
    rows_in = frames.reshape(R, *cfg.img_size)
    provider_ms, provider_reps = median_ms(lambda: ps.parse(rows_in, counts), args.iters, stream)
    tracked_ms, tracked_reps = median_ms(lambda: tk.track(frames, counts), args.iters, stream)
    provider_ms2, provider_reps2 = median_ms(lambda: ps.parse(rows_in, counts), args.iters, stream)
    tracked_ms2, tracked_reps2 = median_ms(lambda: tk.track(frames, counts), args.iters, stream)
    torch.cuda.synchronize()
    tail_ms, tail_reps = median_ms(lambda: eng._replay_or_run(tk._graph, tk._plan), args.iters, eng.stream)
    score_ms, score_reps = median_ms(lambda: eng._replay_or_run(entry["graph"], entry["plan"]), args.iters, eng.stream)
    if opt is not None:
        turns = {"greedy": [], "optimal": []}
        for _ in range(2):
            for name, t in (("greedy", tk), ("optimal", opt)):
                turns[name].append(median_ms(lambda: eng._replay_or_run(t._graph, t._plan), args.iters, eng.stream))
        for name, v in turns.items():
            res["tail_%s_turns_ms" % name] = [m for m, _ in v]
            res["tail_%s_repeats_ms" % name] = [r for _, r in v]
    if id_entry is not None:
        idf_ms, idf_reps = median_ms(lambda: eng._replay_or_run(id_entry["graph"], id_entry["plan"]), args.iters, eng.stream)
        score_ms2, score_reps2 = median_ms(lambda: eng._replay_or_run(entry["graph"], entry["plan"]), args.iters, eng.stream)
        res.update(score_identity_graph_ms=idf_ms, score_identity_repeats_ms=idf_reps, score_graph_again_ms=score_ms2,
                   score_again_repeats_ms=score_reps2)
    res.update(provider_graph_ms=provider_ms, provider_repeats_ms=provider_reps, tracked_graph_ms=tracked_ms, tracked_repeats_ms=tracked_reps,
               provider_graph_again_ms=provider_ms2, provider_again_repeats_ms=provider_reps2, tracked_graph_again_ms=tracked_ms2,
               tracked_again_repeats_ms=tracked_reps2, tail_graph_ms=tail_ms, tail_repeats_ms=tail_reps, score_graph_ms=score_ms,
               score_repeats_ms=score_reps, tail_over_provider=tail_ms / provider_ms, score_over_provider=score_ms / provider_ms,
               tracked_added_ms=tracked_ms - provider_ms, frames_per_s=R / (tracked_ms * 1e-3))
    per = {}
    for _ in range(7):
        for (fn, a, name) in tk._plan + (opt._plan[:1] if opt is not None else []) + (id_entry or entry)["plan"]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, eng._sp()), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    res["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
    if opt is not None:
        res["optimal_over_greedy_associate"] = res["eager_launch_us"]["air_track_associate_optimal"] / res["eager_launch_us"]["air_track_associate"]
        opt.release_graphs()
    tk.release_graphs(); ps.release_graphs()
    return res


def one_chunk_size(args, C):
    from attend_infer_repeat_amd import _lib, track
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R, n_chunks = args.rows, args.stream_chunks
    if R % C:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, C))
    S, T = R // C, int(cfg.max_steps)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    one = track.SequenceTracker(ps, C, birth_score=0.0)
    one.capture()
    st = track.StreamTracker(ps, C, birth_score=0.0)
    st.capture()
    eng, dev = ps.engine, ps.engine.device
    Ft = C * n_chunks
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(Ft)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    host = lambda t: t.cpu().numpy()
    chunk = lambda c: frames[:, c * C:(c + 1) * C].contiguous()
    first = one.track(chunk(0), counts)
    torch.cuda.synchronize()
    first = {k: host(first[k]).copy() for k in ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot", "state_counts", "track_owner")}
    rows, ids = [], []
    for c in range(n_chunks):
        out = st.push(chunk(c), None, counts)
        torch.cuda.synchronize()
        rows.append({k: host(out[k]).copy() for k in ("what", "boxes", "score", "num_objects")})
        ids.append({k: host(out[k]).copy() for k in ("track_id", "obj_state", "prev_frame", "prev_slot", "affinity", "state_counts", "track_owner")})
    same_first = {k: bool((ids[0][k].view(np.uint8) == first[k].view(np.uint8)).all()) for k in first}
    # the one-shot rule on the concatenation: row s * Ft + c * C + f of the whole is row s * C + f of chunk c
    cat = lambda k, tail: np.concatenate([r[k].reshape((T, S, C) + tail) for r in rows], 2).reshape((T, S * Ft) + tail)
    A = rows[0]["what"].reshape(T, R, -1).shape[-1]
    n_all = np.concatenate([r["num_objects"].reshape(S, C) for r in rows], 1).reshape(-1)
    ref = track.reference_associate(np.concatenate([r["what"].reshape(T, S, C, A) for r in rows], 2).reshape(T, S * Ft, A),
                                    cat("boxes", (4,)), cat("score", ()), n_all, Ft, birth_score=0.0, return_margins=True)
    safe = (ref["gate_margin"] >= 1e-9) & (ref["round_margin"] >= 1e-9)
    agree = np.zeros((n_chunks, S), bool)
    for c in range(n_chunks):
        for k in ("track_id", "obj_state", "prev_frame", "prev_slot"):
            want = ref[k].reshape(T, S, Ft)[:, :, c * C:(c + 1) * C]
            ok = (ids[c][k].reshape(T, S, C) == want).all((0, 2))
            agree[c] = ok if k == "track_id" else agree[c] & ok
    share = float(agree[:, safe].mean()) if safe.any() else float("nan")
    res = dict(chunk_frames=C, sequences=S, rows=R, max_steps=T, chunks=n_chunks, sequences_inside_margins=int(safe.sum()),
               chunks_where_stream_and_one_shot_agree=share, first_chunk_equals_one_shot_device=same_first,
               ids_issued=int(host(st.state["seq"])[:, 1].sum()), one_shot_tracks=int(ref["num_tracks"].sum()))
    if share != 1.0 or not all(same_first.values()):
        print(json.dumps(res))
        raise SystemExit("the stream and the one-shot rule disagree: share %r, first chunk %r" % (share, same_first))
    one.track(chunk(0), counts)                                    # the provider's buffers hold chunk 0 for both tails
    torch.cuda.synchronize()
    turns = {"one_shot": [], "stream": []}
    for _ in range(2):
        for name, t in (("one_shot", one), ("stream", st)):
            st.reset()
            torch.cuda.synchronize()
            turns[name].append(median_ms(lambda: eng._replay_or_run(t._graph, t._plan), args.iters, eng.stream))
    for name, v in turns.items():
        res["tail_%s_turns_ms" % name] = [m for m, _ in v]
        res["tail_%s_repeats_ms" % name] = [r for _, r in v]
    # the whole call, provider included: here the rows the tail reads were just written by the parse for both routes (replaying a tail
    # alone leaves the one-shot tail's inputs in the cache, while the stream's state is rewritten by every replay)
    stream = torch.cuda.current_stream()
    calls = {"one_shot": [], "stream": []}
    for _ in range(2):
        st.reset()
        calls["one_shot"].append(median_ms(lambda: one.track(chunk(0), counts), args.iters, stream)[0])
        calls["stream"].append(median_ms(lambda: st.push(chunk(0), None, counts), args.iters, stream)[0])
    res["call_one_shot_turns_ms"], res["call_stream_turns_ms"] = calls["one_shot"], calls["stream"]
    res["stream_over_one_shot_call"] = statistics.median(calls["stream"]) / statistics.median(calls["one_shot"])
    one.track(chunk(0), counts)
    torch.cuda.synchronize()
    res["stream_over_one_shot_tail"] = statistics.median(res["tail_stream_turns_ms"]) / statistics.median(res["tail_one_shot_turns_ms"])
    res["stream_tail_us_per_frame_per_sequence"] = statistics.median(res["tail_stream_turns_ms"]) * 1e3 / C
    per = {}
    for _ in range(7):
        for (fn, a, name) in one._plan[:1] + st._plan:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, eng._sp()), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    res["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
    # what a chunk costs before its first frame and after its last: the same launch with valid = 0 (the state loaded and stored, the
    # padding rows and the retired list written, no `what` row to copy on a restarted stream), and on the live table of the pushes
    # above (valid = 0 again: the state and every live track's slot stored, no row copied either -- none was sighted in the chunk)
    fn, a, name = st._plan[0]
    for label, prepare in (("empty_table", st.reset), ("live_table", lambda: [st.push(chunk(c), None, counts) for c in range(2)])):
        st.reset()
        prepare()
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            st.valid.zero_()
        torch.cuda.synchronize()
        reps = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, eng._sp()), name)
            e1.record(eng.stream)
            e1.synchronize()
            reps.append(e0.elapsed_time(e1) * 1e3)
        res["eager_stream_valid0_%s_us" % label] = statistics.median(reps)
    st.release_graphs(); one.release_graphs(); ps.release_graphs()
    return res


def one_motion_length(args, F, gate=False):
    """--motion: the tracker without motion against the one with it; gate=True (--motion --gate): the motion tracker against the gated
    one"""
    from attend_infer_repeat_amd import _lib, track
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T = R // F, int(cfg.max_steps)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    host = lambda t: t.cpu().numpy()
    res = dict(frames=F, sequences=S, rows=R, max_steps=T)
    base, test = ("motion", "gated") if gate else ("plain", "motion")
    keys = ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot", "pred_where", "pred_boxes") + (("pred_d2",) if gate else ())
    for matching in track.MATCHINGS:
        plain = track.SequenceTracker(ps, F, birth_score=0.0, matching=matching, motion=True if gate else None)
        plain.capture()
        moved = track.SequenceTracker(ps, F, birth_score=0.0, matching=matching, motion=True, motion_gate=True if gate else None)
        moved.capture()
        plain_ids = host(plain.track(frames, counts)["track_id"]).copy()
        out = moved.track(frames, counts)
        torch.cuda.synchronize()
        ref = track.reference_associate_motion(host(out["what"]).reshape(T, R, -1), host(out["where"]).reshape(T, R, 4), host(out["boxes"]),
                                               host(out["score"]), host(out["num_objects"]), F, moved.img_size, birth_score=0.0,
                                               matching=matching, return_margins=True, gate=True if gate else None)
        safe = (ref["gate_margin"] >= 1e-9) & (ref.get("round_margin", np.full(S, np.inf)) >= 1e-9)
        rows = np.repeat(safe, F)
        same = lambda a, b: bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())
        agree = {k: same(host(out[k])[:, rows], ref[k][:, rows]) for k in keys}
        for k in ("num_tracks", "track_first", "track_last", "track_length", "track_gaps", "state_counts"):
            agree[k] = same(host(out[k])[safe], ref[k][safe])
        differ = (host(out["track_id"]) != plain_ids).any(0)
        r = dict(sequences_inside_margins=int(safe.sum()), agreement=agree, tracks=int(ref["num_tracks"].sum()),
                 state_counts=dict(zip(track.STATES, ref["state_counts"].sum(0).tolist())))
        r["tracks_without_the_gate" if gate else "tracks_without_motion"] = int(host(plain.num_tracks).sum())
        r["frames_where_the_gate_changes_an_id" if gate else "frames_where_motion_changes_an_id"] = float(differ.mean())
        res[matching] = r
        if not all(agree.values()):
            print(json.dumps(res))
            raise SystemExit("the %s tracker and the host reference disagree (%s): %r" % (test, matching, agree))
        turns = {base: [], test: []}
        for _ in range(2):
            for name, t in ((base, plain), (test, moved)):
                turns[name].append(median_ms(lambda: eng._replay_or_run(t._graph, t._plan), args.iters, eng.stream))
        for name, v in turns.items():
            r["tail_%s_turns_ms" % name] = [m for m, _ in v]
            r["tail_%s_repeats_ms" % name] = [q for _, q in v]
        for n in (base, test):
            r["tail_%s_ms" % n] = statistics.median(r["tail_%s_turns_ms" % n])
        r["%s_over_%s_tail" % (test, base)] = r["tail_%s_ms" % test] / r["tail_%s_ms" % base]
        per = {}
        for _ in range(7):
            for (fn, a, name) in plain._plan[:1] + moved._plan[:1]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                _lib.check(fn(*a, eng._sp()), name)
                e1.record(eng.stream)
                e1.synchronize()
                per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
        r["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
        plain.release_graphs(); moved.release_graphs()
    ps.release_graphs()
    return res


def one_hota_length(args, F):
    """--hota: air_track_hota beside air_track_score and air_track_idf on the tracks of one captured tracker"""
    from attend_infer_repeat_amd import _lib, track
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T, G = R // F, int(cfg.max_steps), 3
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    tk = track.SequenceTracker(ps, F, birth_score=0.0, matching=args.matching)
    tk.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    out = tk.track(frames, counts)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    boxes, n, ids = host(out["boxes"]), host(out["num_objects"]), host(out["track_id"])
    gt = np.zeros((R, G, 4), np.float32)
    for g in range(G):
        gt[n > g, g] = boxes[g, n > g]
    gt[::5] += np.float32(1.5)                                     # (every fifth frame off its box: the thresholds have work)
    gt_dev = torch.from_numpy(gt).to(dev)
    got = tk.hota(gt_dev, accumulate=False)
    torch.cuda.synchronize()
    n_seq = min(S, args.hota_check)                                # the host reference walks these sequences
    want = track.reference_hota(boxes[:, :n_seq * F], n[:n_seq * F], ids[:, :n_seq * F], gt[:n_seq * F], F, F * T)
    same = lambda a, b: bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())
    keys = ("seq_hota_i", "seq_hota_f", "hota_potential", "hota_id_count", "hota_gt_count", "hota_matches")
    agree = {k: same(host(got[k])[:n_seq], want[k]) for k in keys}
    fig = tk.hota_summary()
    res = dict(frames=F, sequences=S, rows=R, max_steps=T, gt_slots=G, n_ids=F * T, matching=args.matching, sequences_checked=n_seq,
               agreement=agree, hota_summary={k: v for k, v in fig.items() if k != "per_alpha"})
    if not all(agree.values()):
        print(json.dumps(res))
        raise SystemExit("air_track_hota and the host reference disagree: %r" % (agree,))
    tk.score(gt_dev, accumulate=False)
    tk.score(gt_dev, accumulate=False, identity=True)
    res["score_summary"], res["identity_summary"] = tk.summary(), tk.identity_summary()
    graphs = {"score": tk._score[(G, 0.5)], "score_idf": tk._score[(G, 0.5, "idf")], "hota": tk.scores.hota_entries[(G,)]}
    turns = {k: [] for k in graphs}
    for _ in range(2):                                             # in turns, in this process
        for name, e in graphs.items():
            turns[name].append(median_ms(lambda: eng._replay_or_run(e["graph"], e["plan"]), args.iters, eng.stream))
    for name, v in turns.items():
        res["%s_graph_turns_ms" % name] = [m for m, _ in v]
        res["%s_graph_repeats_ms" % name] = [r for _, r in v]
        res["%s_graph_ms" % name] = statistics.median(res["%s_graph_turns_ms" % name])
    res["hota_over_score_graph"] = res["hota_graph_ms"] / res["score_graph_ms"]
    res["hota_over_score_idf_graph"] = res["hota_graph_ms"] / res["score_idf_graph_ms"]
    plan = graphs["score_idf"]["plan"] + graphs["hota"]["plan"]    # air_track_score, air_track_idf, air_track_hota
    launch = lambda fn, a, name: _lib.check(fn(*a, eng._sp()), name)
    eager = {name: [] for _, _, name in plan}
    for _ in range(2):
        for fn, a, name in plan:
            eager[name].append(median_ms(lambda: launch(fn, a, name), args.iters, eng.stream))
    res["eager_launch_us"] = {k: statistics.median([m for m, _ in v]) * 1e3 for k, v in eager.items()}
    res["eager_launch_turns_us"] = {k: [m * 1e3 for m, _ in v] for k, v in eager.items()}
    per = {}
    for _ in range(7):                                             # and one launch at a time between two events, as the other modes time it
        for fn, a, name in plan:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            launch(fn, a, name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    res["eager_single_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
    us = res["eager_launch_us"]
    res["hota_over_score_eager"] = us["air_track_hota"] / us["air_track_score"]
    res["hota_over_score_plus_idf_eager"] = us["air_track_hota"] / (us["air_track_score"] + us["air_track_idf"])
    tk.release_graphs(); ps.release_graphs()
    return res


def one_mots_length(args, F):
    """--mots: air_score_contingency + air_track_mots beside air_track_score on the tracks of one captured tracker"""
    from attend_infer_repeat_amd import _lib, track
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T, G = R // F, int(cfg.max_steps), 3
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    tk = track.SequenceTracker(ps, F, birth_score=0.0, matching=args.matching)
    tk.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    out = tk.track(frames, counts)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    boxes, n, ids, owner = host(out["boxes"]), host(out["num_objects"]), host(out["track_id"]), host(out["owner"])
    inst = np.where(owner < G, owner, -1).astype(np.int8)           # ground truth cut from the parse's own owner map ...
    inst[::5] = np.roll(inst[::5], 2, axis=2)                       # ... every fifth frame two pixels off: those masks miss
    gt = np.zeros((R, G, 4), np.float32)
    for g in range(G):
        gt[n > g, g] = boxes[g, n > g]
    inst_dev, gt_dev = torch.from_numpy(inst).to(dev), torch.from_numpy(gt).to(dev)
    got = tk.mots(inst_dev, G, accumulate=False)
    torch.cuda.synchronize()
    n_seq = min(S, args.mots_check)                                # the host reference walks these sequences
    cont = track.mots_contingency(owner[:n_seq * F], inst[:n_seq * F], T, G)
    want = track.reference_mots(cont, n[:n_seq * F], ids[:, :n_seq * F], F)
    same = lambda a, b: bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())
    agree = {k: same(host(got[k])[:n_seq * (1 if k.startswith("seq") else F)], want[k]) for k in track.MOTS_OUTPUTS}
    agree["cont"] = same(host(got["cont"])[:n_seq * F], cont)
    res = dict(frames=F, sequences=S, rows=R, max_steps=T, gt_slots=G, img_size=list(cfg.img_size), matching=args.matching,
               sequences_checked=n_seq, agreement=agree, mots_summary=tk.mots_summary())
    if not all(agree.values()):
        print(json.dumps(res))
        raise SystemExit("air_track_mots and the host reference disagree: %r" % (agree,))
    tk.score(gt_dev, accumulate=False)
    res["score_summary"] = tk.summary()
    graphs = {"score": tk._score[(G, 0.5)], "mots": tk.scores.mots_entries[(G,)]}
    turns = {k: [] for k in graphs}
    for _ in range(2):                                             # in turns, in this process
        for name, e in graphs.items():
            turns[name].append(median_ms(lambda: eng._replay_or_run(e["graph"], e["plan"]), args.iters, eng.stream))
    for name, v in turns.items():
        res["%s_graph_turns_ms" % name] = [m for m, _ in v]
        res["%s_graph_repeats_ms" % name] = [r for _, r in v]
        res["%s_graph_ms" % name] = statistics.median(res["%s_graph_turns_ms" % name])
    res["mots_over_score_graph"] = res["mots_graph_ms"] / res["score_graph_ms"]
    plan = graphs["score"]["plan"] + graphs["mots"]["plan"]        # air_track_score, air_score_contingency, air_track_mots
    launch = lambda fn, a, name: _lib.check(fn(*a, eng._sp()), name)
    eager = {name: [] for _, _, name in plan}
    for _ in range(2):
        for fn, a, name in plan:
            eager[name].append(median_ms(lambda: launch(fn, a, name), args.iters, eng.stream))
    res["eager_launch_us"] = {k: statistics.median([m for m, _ in v]) * 1e3 for k, v in eager.items()}
    res["eager_launch_turns_us"] = {k: [m * 1e3 for m, _ in v] for k, v in eager.items()}
    per = {}
    for _ in range(7):                                             # and one launch at a time between two events, as the other modes time it
        for fn, a, name in plan:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            launch(fn, a, name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    res["eager_single_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
    us = res["eager_launch_us"]
    res["mots_kernel_over_score_eager"] = us["air_track_mots"] / us["air_track_score"]
    res["mots_pair_over_score_eager"] = (us["air_score_contingency"] + us["air_track_mots"]) / us["air_track_score"]
    tk.release_graphs(); ps.release_graphs()
    return res


def one_stitch_length(args, F):
    """--stitch: the stitcher's captured graph beside the tracker's captured tail, on the tracks of one captured tracker"""
    from attend_infer_repeat_amd import _lib, track
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T = R // F, int(cfg.max_steps)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    tk = track.SequenceTracker(ps, F, birth_score=0.0, matching=args.matching)
    tk.capture()
    st = track.TrackStitcher(tk)
    st.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous().to(dev)
    counts = torch.where((torch.arange(R, device=dev) % F) % 5 < 3, T, 0).to(torch.int32)      # two frames in five empty: the tracks die
    out = st.stitch(frames, counts)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    n_seq = min(S, args.stitch_check)                              # the host reference walks these sequences
    cols = slice(0, n_seq * F)
    want = track.reference_stitch(host(out["what"]).reshape(T, R, -1)[:, cols], host(out["where"]).reshape(T, R, 4)[:, cols],
                                  host(out["track_id"])[:, cols], host(out["num_tracks"])[:n_seq],
                                  *[host(out[k])[:n_seq] for k in ("track_first", "track_last", "track_length", "track_gaps")], F,
                                  appearance_weight=tk.appearance_weight)
    same = lambda a, b: bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())
    agree = {k: same(host(out[k])[:, cols] if k == "stitch_id" else host(out[k])[:n_seq], want[k]) for k in track.STITCH_OUTPUTS}
    tracks, status = host(out["num_tracks"]), host(out["stitch_status"])
    res = dict(frames=F, sequences=S, rows=R, max_steps=T, matching=args.matching, max_gap=st.max_gap, gate=st.gate,
               sequences_checked=n_seq, agreement=agree, tracks=int(tracks.sum()), tracks_per_sequence_max=int(tracks.max()),
               links=int(host(out["num_links"]).sum()), sequences_overflow=int((status == track.STITCH_OVERFLOW).sum()))
    if not all(agree.values()):
        print(json.dumps(res))
        raise SystemExit("air_track_stitch and the host reference disagree: %r" % (agree,))
    graphs = {"tail": tk, "stitch": st}
    turns = {k: [] for k in graphs}
    for _ in range(2):                                             # in turns, in this process
        for name, g in graphs.items():
            turns[name].append(median_ms(lambda: eng._replay_or_run(g._graph, g._plan), args.iters, eng.stream))
    for name, v in turns.items():
        res["%s_graph_turns_ms" % name] = [m for m, _ in v]
        res["%s_graph_repeats_ms" % name] = [r for _, r in v]
        res["%s_graph_ms" % name] = statistics.median(res["%s_graph_turns_ms" % name])
    res["stitch_over_tail_graph"] = res["stitch_graph_ms"] / res["tail_graph_ms"]
    plan = tk._plan + st._plan[:1]                                 # the association entry, air_track_owner, air_track_stitch
    launch = lambda fn, a, name: _lib.check(fn(*a, eng._sp()), name)
    eager = {name: [] for _, _, name in plan}
    for _ in range(2):
        for fn, a, name in plan:
            eager[name].append(median_ms(lambda: launch(fn, a, name), args.iters, eng.stream))
    res["eager_launch_us"] = {k: statistics.median([m for m, _ in v]) * 1e3 for k, v in eager.items()}
    res["eager_launch_turns_us"] = {k: [m * 1e3 for m, _ in v] for k, v in eager.items()}
    res["stitch_over_associate_eager"] = res["eager_launch_us"]["air_track_stitch"] / res["eager_launch_us"][tk._plan[0][2]]
    # where the time goes: the same launch with a gate that admits nothing (the filter walk, the predicts, every d2, the relabel; no msd,
    # and a solver whose rows take their own column at once) and with max_gap = 1 (hardly a candidate: the filter walk and the relabel)
    fn, a, name = st._plan[0]
    at_gap, at_gate = track.STITCH_ARGS.index("max_gap"), track.STITCH_ARGS.index("gate_d2")
    for label, args_ in (("gate_1e-300", a[:at_gate] + (1e-300,) + a[at_gate + 1:]), ("max_gap_1", a[:at_gap] + (1,) + a[at_gap + 1:])):
        res["eager_stitch_%s_us" % label] = median_ms(lambda: launch(fn, args_, name), args.iters, eng.stream)[0] * 1e3
    launch(fn, a, name)                                            # (the outputs of the rule as configured are back)
    st.release_graphs(); tk.release_graphs(); ps.release_graphs()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--matching", choices=("greedy", "optimal"), default="greedy")
    ap.add_argument("--identity", action="store_true")
    ap.add_argument("--stream", type=int, nargs="+", default=None, metavar="CHUNK")
    ap.add_argument("--stream-chunks", type=int, default=4)
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--gate", action="store_true", help="with --motion: the Mahalanobis gate against the motion tracker without it")
    ap.add_argument("--hota", action="store_true", help="air_track_hota beside air_track_score and air_track_idf (eager and captured)")
    ap.add_argument("--hota-check", type=int, default=16, metavar="N", help="with --hota: the sequences the host reference walks")
    ap.add_argument("--stitch", action="store_true", help="the stitcher's captured graph beside the tracker's captured tail")
    ap.add_argument("--stitch-check", type=int, default=16, metavar="N", help="with --stitch: the sequences the host reference walks")
    ap.add_argument("--mots", action="store_true",
                    help="air_score_contingency + air_track_mots beside air_track_score (eager and captured)")
    ap.add_argument("--mots-check", type=int, default=16, metavar="N", help="with --mots: the sequences the host reference walks")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("track_bench measures on the GPU; there is no CPU fallback")
    if args.mots:
        res = dict(tool="track_bench --mots", device=torch.cuda.get_device_name(0), lengths=[one_mots_length(args, F) for F in args.frames])
        print(json.dumps(res))
        for r in res["lengths"]:
            for k, v in r.items():
                print("F=%-4d %-34s %s" % (r["frames"], k, v))
        return res
    if args.stitch:
        res = dict(tool="track_bench --stitch", device=torch.cuda.get_device_name(0), lengths=[one_stitch_length(args, F) for F in args.frames])
        print(json.dumps(res))
        for r in res["lengths"]:
            for k, v in r.items():
                print("F=%-4d %-34s %s" % (r["frames"], k, v))
        return res
    if args.hota:
        res = dict(tool="track_bench --hota", device=torch.cuda.get_device_name(0), lengths=[one_hota_length(args, F) for F in args.frames])
        print(json.dumps(res))
        for r in res["lengths"]:
            for k, v in r.items():
                print("F=%-4d %-34s %s" % (r["frames"], k, v))
        return res
    if args.stream is not None:
        res = dict(tool="track_bench --stream", device=torch.cuda.get_device_name(0), chunks=[one_chunk_size(args, C) for C in args.stream])
        print(json.dumps(res))
        for r in res["chunks"]:
            for k, v in r.items():
                print("CHUNK=%-4d %-40s %s" % (r["chunk_frames"], k, v))
        return res
    if args.gate and not args.motion:
        raise SystemExit("--gate goes with --motion")
    if args.motion:
        res = dict(tool="track_bench --motion" + (" --gate" if args.gate else ""), device=torch.cuda.get_device_name(0),
                   lengths=[one_motion_length(args, F, args.gate) for F in args.frames])
        print(json.dumps(res))
        for r in res["lengths"]:
            for matching in ("greedy", "optimal"):
                for k, v in r[matching].items():
                    print("F=%-4d %-8s %-36s %s" % (r["frames"], matching, k, v))
        return res
    res = dict(tool="track_bench", device=torch.cuda.get_device_name(0), lengths=[one_length(args, F) for F in args.frames])
    print(json.dumps(res))
    for r in res["lengths"]:
        for k, v in r.items():
            print("F=%-4d %-30s %s" % (r["frames"], k, v))
    return res


if __name__ == "__main__":
    main()
