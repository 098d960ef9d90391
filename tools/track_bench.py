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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--matching", choices=("greedy", "optimal"), default="greedy")
    ap.add_argument("--identity", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("track_bench measures on the GPU; there is no CPU fallback")
    res = dict(tool="track_bench", device=torch.cuda.get_device_name(0), lengths=[one_length(args, F) for F in args.frames])
    print(json.dumps(res))
    for r in res["lengths"]:
        for k, v in r.items():
            print("F=%-4d %-30s %s" % (r["frames"], k, v))
    return res


if __name__ == "__main__":
    main()
