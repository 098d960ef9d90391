#!/usr/bin/env python
"""Measurements of best-of-K scene parsing (attend_infer_repeat_amd/particle_parse.py) at the configs[1] shapes (50x50 / 20x20 /
T = 3, A = 50); one JSON line per call.

  the captured ParticleParser.parse() at --images images and --particles K (one hipGraph replay per call, fresh noise) next to
  (a) the captured SceneParser.parse() at the same number of images: the parse a user could get before;
  (b) the captured ImportanceEvaluator.evaluate() at the same (images, K): the K * images-row forward pass with its two read-outs;
  (c) the K * images-row forward plan of the particle parser alone (noise entry included), captured as a graph of its own: the
      difference to the parse is what the added tail costs (log q, reduce, select + gather, spread, objects, render, band sum);
  and the time of every launch of the parse chain issued eagerly (device events around each entry).

Timing: a warm-up, then 5 repeats of --iters calls each; the median repeat is reported.  Device events throughout.  Untrained
parameters: the count head then says n = 0 almost everywhere, so the render draws little -- the forward pass, which dominates, does
not depend on that.  Run each call under its own `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def median_ms(fn, iters, stream):
    fn(); fn()
    torch.cuda.synchronize()
    reps = [timed(fn, iters, stream) * 1e3 for _ in range(5)]
    return statistics.median(reps), reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--particles", type=int, default=16)
    ap.add_argument("--select", default="joint", choices=("joint", "weight"))
    ap.add_argument("--mfma", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.iw_eval import ImportanceEvaluator
    from attend_infer_repeat_amd.parse import SceneParser
    from attend_infer_repeat_amd.particle_parse import ParticleParser
    B, K = args.images, args.particles
    cfg = EngineConfig(mfma_dtype=args.mfma)
    pp = ParticleParser(cfg, B, K, select=args.select, seed=0)
    pp.capture()
    eng = pp.engine
    obs = torch.rand(B, *cfg.img_size, device=eng.device)
    stream = torch.cuda.current_stream()
    parse_ms, parse_reps = median_ms(lambda: pp.parse(obs), args.iters, stream)
    out = pp.parse(obs)
    moved = float((out["best_particle"] != 0).double().mean().item())
    hist = torch.bincount(out["num_objects"].long(), minlength=pp.T + 1).tolist()
    ess = float(out["ess"].double().mean().item())
    # (c) the forward plan alone (with its noise entry), one graph
    fwd_plan = list(eng._plan_fwd_noise)
    g_fwd = eng._capture_plans([fwd_plan])

    def fwd_only():
        eng.wait_for_caller()
        eng._replay_or_run(g_fwd, fwd_plan)
        eng.wait_for_engine()
    fwd_ms, fwd_reps = median_ms(fwd_only, args.iters, stream)
    # per launch, eagerly
    plan, sp = pp._plans[True], eng._sp()
    per = {}
    for _ in range(3):
        for i, (fn, a, name) in enumerate(plan):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, sp), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault("%02d %s" % (i, name), []).append(e0.elapsed_time(e1) * 1e3)
    n_fwd = len(eng._plan_fwd_noise) + 1
    eager = {k: statistics.median(v) for k, v in per.items()}
    tail_eager_us = sum(v for k, v in eager.items() if int(k[:2]) >= n_fwd and "air_iw_logweight" not in k)
    # (a) the deterministic parse, (b) the importance-weighted evaluation
    sp_ = SceneParser(cfg, B, seed=0)
    sp_.capture()
    scene_ms, scene_reps = median_ms(lambda: sp_.parse(obs), args.iters, stream)
    ev = ImportanceEvaluator(cfg, B, K, seed=0)
    ev.capture()
    iw_ms, iw_reps = median_ms(lambda: ev.evaluate(obs), args.iters, stream)
    res = dict(images=B, particles=K, select=args.select, mfma=args.mfma, iters=args.iters, particle_parse_graph_ms=parse_ms,
               images_per_s=B / (parse_ms * 1e-3), repeats_ms=parse_reps, forward_graph_ms=fwd_ms, forward_repeats_ms=fwd_reps,
               tail_ms=parse_ms - fwd_ms, tail_share_of_parse=(parse_ms - fwd_ms) / parse_ms, scene_parse_graph_ms=scene_ms,
               scene_repeats_ms=scene_reps, iw_evaluate_graph_ms=iw_ms, iw_repeats_ms=iw_reps, over_iw_evaluate_ms=parse_ms - iw_ms,
               launches=pp.launch_count(), eager_launch_us=eager, eager_added_tail_us=tail_eager_us, best_particle_moved=moved,
               mean_ess=ess, count_hist=hist)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
