#!/usr/bin/env python
"""Measurements of trajectories on a stream (attend_infer_repeat_amd/trajectory.py: StreamSmoother); prints one JSON line and a table.

For every CHUNK in --chunk (default 8 and 1, the shapes of profiles/track_stream.txt) at --rows provider rows (default 1024: S = rows /
CHUNK sequences of 50 x 50 frames, T = 3): ONE captured SceneParser with untrained parameters and given counts r mod (T + 1); over it
a captured track.StreamTracker (birth_score = 0), a second captured StreamTracker with a captured StreamSmoother(--lag, --horizon)
bound to it, and a captured one-shot SequenceTracker + TrajectorySmoother at F = CHUNK with the same horizon.  The frames of a sequence
are one sparse random image shifted a pixel per frame.

  agreement   --stream-chunks chunks are pushed through the smoother; every tensor of the emitted and the forecast table is compared by
              bytes with trajectory.reference_smooth_stream on the read-back of the same pushes, or the tool exits with an error;
  tails       timed in turns in this process on the engine's stream (tracker, smoother, one-shot smoother, twice): the StreamTracker's
              captured tail (associate + owner), the StreamSmoother's captured graph behind it (stash, smooth, fill and read-out of
              both tables), the TrajectorySmoother's captured graph; the ratios and the smoother's time per frame are reported;
  tail()      the smoother's captured tail graph;
  and every entry of the smoother's plan launched eagerly on its own, summed per part: the smooth kernel (with the stash), the
  emitted table's fill and read-out, the forecast table's fill and read-out.

Replaying the smoother's graph moves its stream on (every replay is a further chunk with the tracker's ids of the last push), which
is what a push does.  Timing: a warm-up, then 5 repeats of --iters calls each between device events; the median repeat is reported."""
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

import attend_infer_repeat_amd  # noqa: E402,F401  (before the first HIP call: the package sets the runtime's graph switches)


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


def one_chunk_size(args, C):
    from attend_infer_repeat_amd import _lib, track, trajectory
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R, n_chunks, lag, Hz = args.rows, args.stream_chunks, args.lag, args.horizon
    if R % C:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, C))
    S, T = R // C, int(cfg.max_steps)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    plain = track.StreamTracker(ps, C, birth_score=0.0)
    plain.capture()
    st = track.StreamTracker(ps, C, birth_score=0.0)
    st.capture()
    sm = trajectory.StreamSmoother(st, lag, Hz)
    sm.capture()
    one = track.SequenceTracker(ps, C, birth_score=0.0)
    one.capture()
    osm = trajectory.TrajectorySmoother(one, Hz)
    osm.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(C * n_chunks)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    host = lambda t: t.detach().cpu().numpy()
    chunk = lambda c: frames[:, c * C:(c + 1) * C].contiguous()
    state, agree, emitted, rows_written = None, True, 0, 0
    for c in range(n_chunks):
        out = sm.push(chunk(c), None, counts)
        torch.cuda.synchronize()
        ref, state = trajectory.reference_smooth_stream(
            state, host(sm._rows["where"]).reshape(T, R, 4), host(ps.num_objects), host(st.track_id), C, None, lag, st.max_age,
            tuple(cfg.img_size), Hz, what=host(sm._rows["what"]).reshape(T, R, -1), glimpse=host(sm._rows["glimpse"]).reshape(T, R, -1),
            score=host(ps.score))
        for k, w in ref.items():
            g = np.ascontiguousarray(host(out[k])).reshape(w.shape)
            agree = agree and g.dtype == w.dtype and bool((g.reshape(-1).view(np.uint8) == np.ascontiguousarray(w).reshape(-1).view(np.uint8)).all())
        emitted += int(ref["num_emitted"].sum())
        rows_written += int(ref["sm_count"].sum())
    res = dict(chunk_frames=C, sequences=S, rows=R, max_steps=T, lag=lag, horizon=Hz, ring_depth=sm.depth, chunks=n_chunks,
               state_bytes=sm.state_bytes, emitted_frames=emitted, emitted_rows=rows_written, emitted_equals_host_reference_bits=agree)
    if not agree:
        print(json.dumps(res))
        raise SystemExit("the stream smoother and the host reference disagree")
    plain.push(chunk(0), None, counts)                             # (valid = CHUNK for the plain tracker's tail too)
    one.track(chunk(0), counts)
    osm.run()
    torch.cuda.synchronize()
    graphs = (("tracker_tail", plain._graph, plain._plan), ("smoother", sm._graph, sm._plan), ("one_shot_smoother", osm._graph, osm._plan))
    turns = {name: [] for name, _, _ in graphs}
    for _ in range(2):
        for name, graph, plan in graphs:
            turns[name].append(median_ms(lambda: eng._replay_or_run(graph, plan), args.iters, eng.stream))
    for name, v in turns.items():
        res["%s_turns_ms" % name] = [m for m, _ in v]
        res["%s_repeats_ms" % name] = [r for _, r in v]
    med = {name: statistics.median(res["%s_turns_ms" % name]) for name in turns}
    res.update(smoother_over_tracker_tail=med["smoother"] / med["tracker_tail"],
               smoother_over_one_shot_smoother=med["smoother"] / med["one_shot_smoother"],
               smoother_us_per_frame=med["smoother"] * 1e3 / C, one_shot_smoother_us_per_frame=med["one_shot_smoother"] * 1e3 / C)
    res["tail_call_graph_ms"], res["tail_call_repeats_ms"] = median_ms(lambda: eng._replay_or_run(sm._tail["graph"], sm._tail["plan"]),
                                                                       args.iters, eng.stream)
    per = {}
    for _ in range(7):
        for seg, entries in sm.segments.items():
            for (fn, a, name) in entries:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                _lib.check(fn(*a, eng._sp()), name)
                e1.record(eng.stream)
                e1.synchronize()
                per.setdefault("%s:%s" % (seg, name), []).append(e0.elapsed_time(e1) * 1e3)
    eager = {k: statistics.median(v) for k, v in per.items()}
    part = lambda *segs: sum(v for k, v in eager.items() if k.split(":")[0] in segs)
    res["eager_launch_us"] = eager
    res["eager_parts_us"] = dict(smooth_and_stash=part("stash", "smooth"), emitted_fill_and_readout=part("fill", "readout"),
                                 forecast_fill_and_readout=part("fill_forecast", "readout_forecast"))
    for s in (sm, osm, st, one, plain, ps):
        s.release_graphs()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--lag", type=int, default=2)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stream-chunks", type=int, default=4)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_stream_bench measures on the GPU; there is no CPU fallback")
    res = dict(tool="trajectory_stream_bench", device=torch.cuda.get_device_name(0), chunks=[one_chunk_size(args, C) for C in args.chunk])
    print(json.dumps(res))
    for r in res["chunks"]:
        for k, v in r.items():
            print("CHUNK=%-4d %-40s %s" % (r["chunk_frames"], k, v))
    return res


if __name__ == "__main__":
    main()
