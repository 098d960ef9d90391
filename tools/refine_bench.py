#!/usr/bin/env python
"""Measurements of parse refinement (attend_infer_repeat_amd/refine.py) at the configs[1] shapes (50x50 / 20x20 / T = 3, A = 50); one
JSON line per mode.

  --mode time     the captured ParseRefiner.parse() at --images images and N in --steps (the parser's graph replay + the refiner's)
                  next to the captured bound parser alone; and every launch of the N = 1 chain issued eagerly (device events around
                  each entry): one iteration's forward, backward and step, and the closing evaluation.  Untrained parameters with
                  given counts t mod (T + 1), so that every count renders.
  --mode quality  one short training run on the procedural glyphs (scripts/multi_mnist.py --glyphs, --train-iters updates), then on
                  its annotated validation set: count accuracy / mAP / foreground ARI of the parse at the mode without refinement and
                  with N = --quality-steps iterations at refine.DEFAULT_LR, and the sweep the default learning rates are chosen from --
                  lr_what x lr_where over --sweep (one decade either side of 1e-2 by default), judged by the mean objective gain.

Timing: a warm-up, then 5 repeats of --iters calls each; the median repeat is reported.  Device events throughout.  Run each call
under its own `timeout`."""
import argparse
import json
import os
import statistics
import sys
import tempfile

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


def time_mode(args):
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    from attend_infer_repeat_amd.refine import DEFAULT_LR, ParseRefiner
    B = args.images
    cfg = EngineConfig()
    ps = SceneParser(cfg, B, seed=0)
    ps.capture()
    obs = torch.rand(B, *cfg.img_size, device=ps.engine.device)
    counts = (torch.arange(B, device=ps.engine.device) % (ps.T + 1)).to(torch.int32)
    stream = torch.cuda.current_stream()
    base_ms, base_reps = median_ms(lambda: ps.parse(obs, counts), args.iters, stream)
    res = dict(mode="time", images=B, iters=args.iters, lr=list(DEFAULT_LR), parser_graph_ms=base_ms, parser_repeats_ms=base_reps,
               refine={})
    for n in args.steps:
        rf = ParseRefiner(ps, n, *DEFAULT_LR)
        rf.capture()
        ms, reps = median_ms(lambda: rf.parse(obs, counts), args.iters, stream)
        out = rf.parse(obs, counts)
        gain = torch.nan_to_num(out["objective"] - out["objective_start"].double(), nan=0.0).mean().item()
        res["refine"][str(n)] = dict(graph_ms=ms, repeats_ms=reps, added_ms=ms - base_ms, per_iteration_ms=(ms - base_ms) / max(n, 1),
                                     images_per_s=B / (ms * 1e-3), launches=rf.launch_count(), objective_gain=gain,
                                     moved=float((out["best_iter"] > 0).double().mean().item()))
        rf.release_graphs()
    # every launch of the N = 1 chain, eagerly
    rf = ParseRefiner(ps, 1, *DEFAULT_LR)
    ps.parse(obs, counts)
    sp, eng, per = ps.engine._sp(), ps.engine, {}
    for _ in range(5):
        for i, (fn, a, name) in enumerate(rf._plan):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, sp), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault("%02d %s" % (i, name), []).append(e0.elapsed_time(e1) * 1e3)
    res["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
    return res


def quality_mode(args):
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.refine import DEFAULT_LR
    from attend_infer_repeat_amd.scripts import multi_mnist
    with tempfile.TemporaryDirectory() as tmp:
        air = multi_mnist.main(["--glyphs", "--iters", str(args.train_iters), "--log-every", str(args.train_iters), "--save-every",
                                str(10 * args.train_iters), "--synthetic-samples", str(args.train_samples), "--eval-batches", "1",
                                "--summary-every", "0", "--results-dir", tmp, "--data-dir", os.path.join(tmp, "none"),
                                "--device-feeder", "--seed", str(args.seed)])
    B, N = int(air.obs.shape[0]), args.quality_steps
    d = procedural_multi_mnist(B * args.eval_batches, seed=args.seed + 1000, return_annotations=True)
    imgs = torch.as_tensor(d["imgs"].astype("float32") / 255.0).cuda()
    G = int(d["boxes"].shape[1])

    def run(**kw):
        scorer = air.parse_scorer(G, **kw)
        scorer.reset()
        gain = moved = 0.0
        for i in range(args.eval_batches):
            sl = slice(i * B, (i + 1) * B)
            air.score_parse(imgs[sl], torch.as_tensor(d["instances"][sl]), torch.as_tensor(d["boxes"][sl]), **kw)
            if kw:
                o = air.parsed
                gain += torch.nan_to_num(o["objective"] - o["objective_start"].double(), nan=0.0).sum().item()
                moved += (o["best_iter"] > 0).double().sum().item()
        s = scorer.summary()
        out = {k: s[k] for k in ("count_acc", "map", "fg_ari", "mean_best_overlap", "matched_box_iou")}
        if kw:
            out.update(objective_gain=gain / (B * args.eval_batches), refine_moved=moved / (B * args.eval_batches))
        return out

    res = dict(mode="quality", train_iters=args.train_iters, images=B * args.eval_batches, steps=N, default_lr=list(DEFAULT_LR),
               mode_parse=run(), refined_default=run(refine=N, refine_lr=DEFAULT_LR), sweep=[])
    for lw in args.sweep:
        for lh in args.sweep:
            res["sweep"].append(dict(lr_what=lw, lr_where=lh, **run(refine=N, refine_lr=(lw, lh))))
    best = max(res["sweep"], key=lambda r: r["objective_gain"])
    res["best_by_objective_gain"] = dict(lr_what=best["lr_what"], lr_where=best["lr_where"], objective_gain=best["objective_gain"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "quality"))
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--steps", type=int, nargs="+", default=[0, 4, 16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-iters", type=int, default=20000)
    ap.add_argument("--train-samples", type=int, default=6000)
    ap.add_argument("--eval-batches", type=int, default=4)
    ap.add_argument("--quality-steps", type=int, default=16)
    ap.add_argument("--sweep", type=float, nargs="+", default=[1e-3, 1e-2, 1e-1])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    res = time_mode(args) if args.mode == "time" else quality_mode(args)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
