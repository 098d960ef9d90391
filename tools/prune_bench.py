#!/usr/bin/env python
"""Measurements of subset pruning (attend_infer_repeat_amd/prune.py); one JSON line per mode.

  --mode time     the captured ParsePruner.parse() behind a captured SceneParser at --images images, for the configs[1] shapes
                  (50x50 / 20x20 / T = 3) and the configs[3] shapes (100x100 / 28x28 / T = 5), both candidate modes, next to the
                  captured parser alone; and every launch of the pruner's list issued eagerly (device events around each entry), so
                  that air_prune_score stands next to air_parse_render on the same rows.  Untrained parameters with given counts
                  t mod (T + 1), so that every count occurs.
  --mode quality  one short training run on the procedural glyphs (scripts/multi_mnist.py --glyphs, --train-iters updates), then on
                  its annotated validation set: count accuracy / mAP / foreground ARI of the parse at the mode without pruning and
                  with prune="present" / "all", and the shares of images whose count changed.

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


SHAPES = {"c2": dict(), "c4": dict(img_size=(100, 100), crop_size=(28, 28), max_steps=5)}


def time_mode(args):
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    from attend_infer_repeat_amd.prune import ParsePruner
    B = args.images
    res = dict(mode="time", images=B, iters=args.iters, shapes={})
    stream = torch.cuda.current_stream()
    for tag in args.shapes:
        cfg = EngineConfig(**SHAPES[tag])
        ps = SceneParser(cfg, B, seed=0)
        ps.capture()
        obs = torch.rand(B, *cfg.img_size, device=ps.engine.device)
        counts = (torch.arange(B, device=ps.engine.device) % (ps.T + 1)).to(torch.int32)
        base_ms, base_reps = median_ms(lambda ps=ps: ps.parse(obs, counts), args.iters, stream)
        r = dict(T=ps.T, img=list(cfg.img_size), crop=list(cfg.crop_size), parser_graph_ms=base_ms, parser_repeats_ms=base_reps)
        for cand in ("present", "all"):
            pr = ParsePruner(ps, cand)
            pr.capture()
            ms, reps = median_ms(lambda pr=pr: pr.parse(obs, counts), args.iters, stream)
            out = pr.parse(obs, counts)
            gain = torch.nan_to_num(out["objective"] - out["objective_start"], nan=0.0, posinf=0.0, neginf=0.0).mean().item()
            r[cand] = dict(graph_ms=ms, repeats_ms=reps, added_ms=ms - base_ms, images_per_s=B / (ms * 1e-3), n_bands=pr.n_bands,
                           count_changed=float((out["num_objects"] != out["num_objects_start"]).double().mean().item()),
                           objective_gain=gain)
            pr.release_graphs()
            # every launch of the list, eagerly
            ps.parse(obs, counts)
            sp, eng, per = ps.engine._sp(), ps.engine, {}
            for _ in range(7):
                for i, (fn, a, name) in enumerate(pr._plan):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(eng.stream)
                    _lib.check(fn(*a, sp), name)
                    e1.record(eng.stream)
                    e1.synchronize()
                    per.setdefault("%02d %s" % (i, name), []).append(e0.elapsed_time(e1) * 1e3)
            r[cand]["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
        ps.release_graphs()
        res["shapes"][tag] = r
    return res


def quality_mode(args):
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.scripts import multi_mnist
    with tempfile.TemporaryDirectory() as tmp:
        air = multi_mnist.main(["--glyphs", "--iters", str(args.train_iters), "--log-every", str(args.train_iters), "--save-every",
                                str(10 * args.train_iters), "--synthetic-samples", str(args.train_samples), "--eval-batches", "1",
                                "--summary-every", "0", "--results-dir", tmp, "--data-dir", os.path.join(tmp, "none"),
                                "--device-feeder", "--seed", str(args.seed)])
    B = int(air.obs.shape[0])
    d = procedural_multi_mnist(B * args.eval_batches, seed=args.seed + 1000, return_annotations=True)
    imgs = torch.as_tensor(d["imgs"].astype("float32") / 255.0).cuda()
    G = int(d["boxes"].shape[1])

    def run(**kw):
        scorer = air.parse_scorer(G, **kw)
        scorer.reset()
        tot = torch.zeros(4, dtype=torch.float64, device=imgs.device)
        for i in range(args.eval_batches):
            sl = slice(i * B, (i + 1) * B)
            air.score_parse(imgs[sl], torch.as_tensor(d["instances"][sl]), torch.as_tensor(d["boxes"][sl]), **kw)
            if kw:
                from attend_infer_repeat_amd.evaluation import _prune_sums
                tot += torch.stack(_prune_sums(air.parsed))
        s = scorer.summary()
        out = {k: s[k] for k in ("count_acc", "map", "fg_ari", "mean_best_overlap", "matched_box_iou")}
        if kw:
            out.update(zip(("count_changed", "objects_dropped", "objects_added", "objective_gain"), (tot / (B * args.eval_batches)).tolist()))
        return out

    return dict(mode="quality", train_iters=args.train_iters, seed=args.seed, images=B * args.eval_batches, mode_parse=run(),
                pruned_present=run(prune="present"), pruned_all=run(prune="all"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "quality"))
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--shapes", nargs="+", default=["c2", "c4"], choices=sorted(SHAPES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-iters", type=int, default=20000)
    ap.add_argument("--train-samples", type=int, default=6000)
    ap.add_argument("--eval-batches", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    res = time_mode(args) if args.mode == "time" else quality_mode(args)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
