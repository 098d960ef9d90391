#!/usr/bin/env python
"""Measurements of residual proposals (attend_infer_repeat_amd/propose.py); one JSON line per mode.

  --mode time     the captured ParseProposer.parse() behind a captured SceneParser at --images images, next to the captured
                  ParsePruner.parse(candidates="all") behind the same parser (what the parse cost before proposals existed) and the
                  captured parser alone: the configs[1] shapes (50x50 / 20x20 / T = 3) with P = 1 and P = 3, rounds = 1 and 2, and the
                  configs[3] shapes (100x100 / 28x28 / T = 5) with P = 1.  And air_propose_residual issued eagerly next to
                  air_parse_render on the same rows (device events around each entry): the residual kernel writes one float per
                  pixel where the renderer writes the reconstruction, the owner map and the areas; the ratio is reported.  Untrained
                  parameters with given counts t mod (T + 1), so that every count occurs.
  --mode quality  one short training run on the procedural glyphs (scripts/multi_mnist.py --glyphs, --train-iters updates), then on
                  its annotated validation set: count accuracy / mAP / foreground ARI of the parse at the mode, with prune="all", and
                  with propose=1, (1, 2) and 3; the share of images that gained an object from the residual, the share whose count
                  changed, and the mean objective gain.

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


SHAPES = {"c2": (dict(), ((1, 1), (1, 2), (3, 1), (3, 2))),
          "c4": (dict(img_size=(100, 100), crop_size=(28, 28), max_steps=5), ((1, 1),))}


def eager_us(eng, entries, repeats=9):
    """median device time of each entry of a launch list, issued eagerly one at a time"""
    from attend_infer_repeat_amd import _lib
    sp, per = eng._sp(), {}
    for _ in range(repeats):
        for fn, a, name in entries:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, sp), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in per.items()}


def time_mode(args):
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    from attend_infer_repeat_amd.propose import ParseProposer
    from attend_infer_repeat_amd.prune import ParsePruner
    B = args.images
    res = dict(mode="time", images=B, iters=args.iters, shapes={})
    stream = torch.cuda.current_stream()
    for tag in args.shapes:
        kw, specs = SHAPES[tag]
        cfg = EngineConfig(**kw)
        ps = SceneParser(cfg, B, seed=0)
        ps.capture()
        obs = torch.rand(B, *cfg.img_size, device=ps.engine.device)
        counts = (torch.arange(B, device=ps.engine.device) % (ps.T + 1)).to(torch.int32)
        base_ms, base_reps = median_ms(lambda ps=ps: ps.parse(obs, counts), args.iters, stream)
        r = dict(T=ps.T, img=list(cfg.img_size), crop=list(cfg.crop_size), parser_graph_ms=base_ms, parser_repeats_ms=base_reps)
        pr = ParsePruner(ps, "all")
        pr.capture()
        prune_ms, prune_reps = median_ms(lambda pr=pr: pr.parse(obs, counts), args.iters, stream)
        r["prune_all"] = dict(graph_ms=prune_ms, repeats_ms=prune_reps)
        pr.release_graphs()
        for P, rounds in specs:
            pp = ParseProposer(ps, P, rounds)
            pp.capture()
            ms, reps = median_ms(lambda pp=pp: pp.parse(obs, counts), args.iters, stream)
            out = pp.parse(obs, counts)
            torch.cuda.synchronize()
            gain = torch.nan_to_num(out["objective"] - out["objective_start"], nan=0.0, posinf=0.0, neginf=0.0).mean().item()
            d = dict(graph_ms=ms, repeats_ms=reps, added_ms=ms - base_ms, over_prune_all=ms / prune_ms, images_per_s=B / (ms * 1e-3),
                     n_bands=pp.n_bands, launches=len(pp._plan),
                     count_changed=float((out["num_objects"] != out["num_objects_start"]).double().mean().item()),
                     gained_from_residual=float((out["objects_proposed_kept"] > 0).double().mean().item()), objective_gain=gain)
            pp.release_graphs()
            if (P, rounds) == specs[0]:                            # the residual kernel next to the renderer, on the same rows
                ps.parse(obs, counts)
                torch.cuda.synchronize()
                per = eager_us(ps.engine, [pp.segments[0]["residual"][0], ps._plans[True][-2]])
                per["residual_over_render"] = per["air_propose_residual"] / per["air_parse_render"]
                d["eager_launch_us"] = per
                d["eager_segments_us"] = {name: sum(eager_us(ps.engine, pp.segments[0][name], 5).values())
                                          for name in ("residual", "forward", "pool", "score", "select", "source")}
            r["P%d_R%d" % (P, rounds)] = d
        ps.release_graphs()
        res["shapes"][tag] = r
    return res


def quality_mode(args):
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.evaluation import _propose_sums
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
            if "propose" in kw:
                out = air.parsed
                tot += torch.stack(_propose_sums(out) + [(out["objects_proposed_kept"] > 0).double().sum()])
        s = scorer.summary()
        out = {k: s[k] for k in ("count_acc", "map", "fg_ari", "mean_best_overlap", "matched_box_iou")}
        if "propose" in kw:
            out.update(zip(("objects_added_from_residual", "count_changed", "objective_gain", "images_gained_an_object"),
                           (tot / (B * args.eval_batches)).tolist()))
        return out

    return dict(mode="quality", train_iters=args.train_iters, seed=args.seed, images=B * args.eval_batches, mode_parse=run(),
                pruned_all=run(prune="all"), proposed_1=run(propose=1), proposed_1x2=run(propose=(1, 2)), proposed_3=run(propose=3))


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
