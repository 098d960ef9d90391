#!/usr/bin/env python
"""Measurements of the trajectory smoother (attend_infer_repeat_amd/trajectory.py); prints one JSON line and a readable table.

The configuration of tools/track_bench.py: for every F in --frames (default 8 and 32) at --rows provider rows (default 1024: S = rows / F
sequences of 50 x 50 frames, T = 3), a captured SceneParser with untrained parameters and given counts r mod (T + 1), a captured
SequenceTracker over it with birth_score = 0, and for every horizon in --horizons (default 0 and 4) a captured TrajectorySmoother over
that tracker.  The frames of a sequence are one sparse random image shifted a pixel per frame.

  agreement   the smoother's tables (and the filled rows) against trajectory.reference_smooth on the read-back of the same call, every
              element, floats by their bits (a NaN by its position): they must agree exactly, or the tool exits with an error;
  provider    the provider's own captured parse() of the R rows;
  tracker     the tracker's own graph alone (air_track_associate + air_track_owner);
  trajectory  the smoother's own graph alone (air_track_smooth, air_track_fill and the read-out kernels, both tables);
  and every entry of the smoother's launch list launched eagerly on its own.

--fit measures the noise fitter (trajectory.TrajectoryNoiseFitter) instead, at the same shapes: for every G in --candidates (default 1, 8,
19, 32; log-spaced ratios from 1e-6 to 1e3) a captured fitter over the same tracker --

  agreement   the fitter's per-sequence statistics and totals against trajectory.reference_noise_stats on the read-back of the same
              call, by their bits: they must agree exactly, or the tool exits with an error;
  fit         the fitter's own graph alone (air_track_noise_stats + air_track_noise_reduce);
  smooth_rule air_track_smooth alone (eager launches back to back) and the smoother's whole graph at horizon 0: the only other way to
              the same information is one smoother graph (and a scoring graph) per candidate, so G smoother-rule launches are its
              floor; the tool exits with an error if the fitter at G = 19 does not stay under 19 of them.

Timing: a warm-up, then 5 repeats of --iters calls each between device events; the median repeat is reported with all repeats."""
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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return bool(a.dtype == b.dtype and np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def one_length(args, F):
    from attend_infer_repeat_amd import _lib, track, trajectory
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T = R // F, int(cfg.max_steps)
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
    rows_in = frames.reshape(R, *cfg.img_size)
    host = lambda t: t.cpu().numpy()
    res = dict(frames=F, sequences=S, rows=R, max_steps=T, horizons=[])
    provider_ms, provider_reps = median_ms(lambda: ps.parse(rows_in, counts), args.iters, stream)
    base = tk.track(frames, counts)
    torch.cuda.synchronize()
    tracker_ms, tracker_reps = median_ms(lambda: eng._replay_or_run(tk._graph, tk._plan), args.iters, eng.stream)
    res.update(provider_graph_ms=provider_ms, provider_repeats_ms=provider_reps, tracker_graph_ms=tracker_ms,
               tracker_repeats_ms=tracker_reps, tracks=int(base["num_tracks"].sum()))
    for Hz in args.horizons:
        sm = trajectory.TrajectorySmoother(tk, horizon=Hz)
        sm.capture()
        out = sm.run(tk.track(frames, counts))
        torch.cuda.synchronize()
        ref = trajectory.reference_smooth(host(sm._rows["where"]).reshape(T, R, 4), host(ps.num_objects), host(tk.track_id),
                                          host(tk.num_tracks), host(tk.track_first), host(tk.track_last), F, tk.max_age, cfg.img_size, Hz,
                                          what=host(sm._rows["what"]).reshape(T, R, -1),
                                          glimpse=host(sm._rows["glimpse"]).reshape(T, R, -1), score=host(ps.score))
        agree = {k: same_bits(host(out[k]).reshape(v.shape), v) for k, v in ref.items() if k in out}
        h = dict(horizon=Hz, completed_rows=sm.C, agreement=agree, workspace_bytes=sm.workspace_bytes,
                 rows_per_state=dict(zip(trajectory.STATES[:3], ref["sm_counts"].sum(0).tolist())),
                 forecast_rows=int(ref["fc_count"].sum()) if Hz else 0)
        if not all(agree.values()):
            print(json.dumps(h))
            raise SystemExit("the smoother and the host reference disagree: %r" % ({k: v for k, v in agree.items() if not v},))
        ms, reps = median_ms(lambda: eng._replay_or_run(sm._graph, sm._plan), args.iters, eng.stream)
        h.update(trajectory_graph_ms=ms, trajectory_repeats_ms=reps, trajectory_over_provider=ms / provider_ms,
                 trajectory_over_tracker=ms / tracker_ms)
        per = {}
        for _ in range(7):
            for seg, plan in sm.segments.items():
                for (fn, a, name) in plan:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(eng.stream)
                    _lib.check(fn(*a, eng._sp()), name)
                    e1.record(eng.stream)
                    e1.synchronize()
                    per.setdefault(seg + ":" + name, []).append(e0.elapsed_time(e1) * 1e3)
        h["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
        h["smooth_us_per_frame"] = h["eager_launch_us"]["smooth:air_track_smooth"] / F
        sm.release_graphs()
        res["horizons"].append(h)
    tk.release_graphs(); ps.release_graphs()
    return res


def fit_length(args, F):
    """--fit: the fitter's graph at every G of --candidates, the smoother-rule launch and the smoother's graph at the same shape"""
    from attend_infer_repeat_amd import _lib, track, trajectory
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    R = args.rows
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T = R // F, int(cfg.max_steps)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    tk = track.SequenceTracker(ps, F, birth_score=0.0)
    tk.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    frames = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    host = lambda t: t.cpu().numpy()
    base = tk.track(frames, counts)
    torch.cuda.synchronize()
    sm = trajectory.TrajectorySmoother(tk, horizon=0)
    sm.capture()
    sm.run(base)
    torch.cuda.synchronize()
    graph_ms, graph_reps = median_ms(lambda: eng._replay_or_run(sm._graph, sm._plan), args.iters, eng.stream)
    fn, a, name = sm.segments["smooth"][0]
    rule_ms, rule_reps = median_ms(lambda: _lib.check(fn(*a, eng._sp()), name), args.iters, eng.stream)
    res = dict(frames=F, sequences=S, rows=R, max_steps=T, tracks=int(base["num_tracks"].sum()), smoother_graph_ms=graph_ms,
               smoother_graph_repeats_ms=graph_reps, smooth_rule_ms=rule_ms, smooth_rule_repeats_ms=rule_reps, candidates=[])
    sm.release_graphs()
    for G in args.candidates:
        grid = tuple(float(v) for v in np.geomspace(1e-6, 1e3, G)) if G > 1 else (0.25,)
        ft = trajectory.TrajectoryNoiseFitter(tk, grid, grid)
        ft.capture()
        ft.run(accumulate=False)
        torch.cuda.synchronize()
        ref = trajectory.reference_noise_stats(host(ft._where).reshape(T, R, 4), host(ps.num_objects), host(tk.track_id), host(tk.num_tracks),
                                               host(tk.track_first), host(tk.track_last), F, grid, grid, ft.velocity_ratio)
        got = dict({k: host(v) for k, v in ft.stats.items()}, **ft.read_totals())
        bits = lambda v: np.ascontiguousarray(v).view(np.uint64) if v.dtype == np.float64 else v
        agree = {k: bool(got[k].dtype == ref[k].dtype and np.array_equal(bits(got[k]), bits(ref[k]))) for k in got}
        c = dict(G=G, agreement=agree, updates=int(ref["n"].sum()))
        if not all(agree.values()):
            print(json.dumps(c))
            raise SystemExit("the fitter and the host reference disagree: %r" % ({k: v for k, v in agree.items() if not v},))
        ms, reps = median_ms(lambda: eng._replay_or_run(ft._graph, ft._plan), args.iters, eng.stream)
        c.update(fit_graph_ms=ms, fit_repeats_ms=reps, fit_over_smooth_rule=ms / rule_ms, floor_of_the_alternative_ms=G * rule_ms,
                 one_smoother_graph_per_candidate_ms=G * graph_ms, one_smoother_graph_per_pair_ms=G * G * graph_ms)
        per = {}
        for _ in range(7):
            for (efn, ea, ename) in ft._plan:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                _lib.check(efn(*ea, eng._sp()), ename)
                e1.record(eng.stream)
                e1.synchronize()
                per.setdefault(ename, []).append(e0.elapsed_time(e1) * 1e3)
        c["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
        try:
            fit = ft.fit()
            c["fit"] = {k: fit[k] for k in ("process_noise", "measurement_noise", "velocity_var", "cell", "on_edge")}
            c["loglik_per_innovation"] = fit["loglik"] / fit["n_innovations"]
        except ValueError as e:
            c["fit"] = str(e)
        ft.release_graphs()
        res["candidates"].append(c)
        if G == 19 and not ms < 19 * rule_ms:
            print(json.dumps(res))
            raise SystemExit("the fitter at G = 19 took %.4f ms, 19 smoother-rule launches %.4f ms" % (ms, 19 * rule_ms))
    tk.release_graphs(); ps.release_graphs()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--horizons", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fit", action="store_true", help="measure the noise fitter instead of the smoother")
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 8, 19, 32])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_bench measures on the GPU; there is no CPU fallback")
    if args.fit:
        res = dict(tool="trajectory_bench --fit", device=torch.cuda.get_device_name(0), lengths=[fit_length(args, F) for F in args.frames])
        print(json.dumps(res))
        for r in res["lengths"]:
            for k, v in r.items():
                if k != "candidates":
                    print("F=%-4d %-36s %s" % (r["frames"], k, v))
            for c in r["candidates"]:
                for k, v in c.items():
                    print("F=%-4d G=%-2d %-33s %s" % (r["frames"], c["G"], k, v))
        return res
    res = dict(tool="trajectory_bench", device=torch.cuda.get_device_name(0), lengths=[one_length(args, F) for F in args.frames])
    print(json.dumps(res))
    for r in res["lengths"]:
        for k, v in r.items():
            if k != "horizons":
                print("F=%-4d %-30s %s" % (r["frames"], k, v))
        for h in r["horizons"]:
            for k, v in h.items():
                print("F=%-4d Hz=%-2d %-27s %s" % (r["frames"], h["horizon"], k, v))
    return res


if __name__ == "__main__":
    main()
