#!/usr/bin/env python
"""Step time of training on the K-particle importance-weighted bound (AIRonMNIST.train_step(iw_samples=K), the generic autograd path)
next to the default objective on the SAME generic path (use_engine=False) at the same number of rows, and the eager time of the two
launches the objective adds (air_iw_logweight_bwd, air_iw_vimco).  The fused engine is not the comparison: the K-particle objective
does not run on it.  `--objective rws`: the reweighted wake-sleep objective (iw_objective="rws") beside the VIMCO objective instead, and
the eager time of air_iw_logposterior_bwd (with and without the sample gradients) beside air_iw_logweight_bwd.

  python tools/iw_train_bench.py [--images 64] [--particles 2 5] [--steps 40] [--warmup 10] [--repeats 3] [--objective rws]

Host clock around `steps` updates that end in a device synchronise; the variants alternate inside every repeat.  One JSON line per
figure on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def make_model(rows, iw_samples, seed=0, iw_objective=None):
    from attend_infer_repeat_amd import mnist_model, utils
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    AD = utils.AttrDict
    imgs, nums = synthetic_multi_mnist(rows, (50, 50), 2, seed=seed)
    x, y = torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda()
    torch.manual_seed(seed)
    air = mnist_model.AIRonMNIST(x, y, max_steps=3, explore_eps=1e-3, steps_pred_hidden=[128, 64], transform_var_bias=.5,
                                 step_bias=.75, output_multiplier=.5)
    nsp = AD(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    ts, _ = air.train_step(1e-4, 0., AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp, use_engine=False,
                           iw_samples=iw_samples, **({} if iw_objective is None else dict(iw_objective=iw_objective)))
    assert air._engine is None
    return lambda: ts(x, y)


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def launch_times(R, K, iters=200, T=3, A=50):
    """eager microseconds per call of the two new entries at R rows (device events around `iters` calls)"""
    from attend_infer_repeat_amd import hip as H
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    what, what_loc, where, where_loc = rn(T, R, A), rn(T, R, A), rn(T, R, 4), rn(T, R, 4)
    what_scale, where_scale = rn(T, R, A).abs() + 0.3, rn(T, R, 4).abs() + 0.3
    presence = (torch.rand(T, R, device="cuda", generator=g) < 0.7).float().cumprod(0)
    gr, logw = rn(R), rn(R) * 10 - 700
    pr = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    out = {}
    latents = (what, what_loc, what_scale, where, where_loc, where_scale, presence)
    for name, fn in (("air_iw_logweight_bwd", lambda: H.iw_logweight_bwd(*latents, gr, K, pr)),
                     ("air_iw_vimco", lambda: H.iw_vimco(logw, K)),
                     ("air_iw_logposterior_bwd", lambda: H.iw_logposterior_bwd(*latents, gr, K)),
                     ("air_iw_logposterior_bwd_fixed_samples", lambda: H.iw_logposterior_bwd(*latents, gr, K, want_what=False,
                                                                                             want_where=False))):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) / iters * 1e3
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--particles", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--objective", choices=("vimco", "rws"), default="vimco",
                    help="rws: time train_step(iw_samples=K, iw_objective='rws') beside the VIMCO objective (iw_objective not given: the "
                         "code path without the option) in the same run, alternating, instead of beside the default objective")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("iw_train_bench needs a GPU: a CPU run gives no time")
    for K in args.particles:
        rows = args.images * K
        if args.objective == "rws":
            variants = {"iw_rws": make_model(args.images, K, iw_objective="rws"), "iw_train": make_model(args.images, K)}
        else:
            variants = {"iw_train": make_model(args.images, K), "default_generic": make_model(rows, None)}
        for step in variants.values():
            for _ in range(args.warmup):
                step()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, step in variants.items():                        # alternating: the two share whatever the host is doing
                ms[k].append(timed(step, args.steps))
        for k, v in ms.items():
            tiled = k != "default_generic"
            print(json.dumps(dict(figure="ms_per_update", variant=k, images=args.images if tiled else rows, particles=K if tiled else None,
                                  rows=rows, median=sorted(v)[len(v) // 2], runs=v, steps=args.steps)), flush=True)
        if args.objective == "rws":
            a, b = sorted(ms["iw_rws"]), sorted(ms["iw_train"])
            print(json.dumps(dict(figure="rws_over_vimco", particles=K, ratio_of_medians=a[len(a) // 2] / b[len(b) // 2],
                                  spread_rws=(a[-1] - a[0]) / a[len(a) // 2], spread_vimco=(b[-1] - b[0]) / b[len(b) // 2])), flush=True)
        print(json.dumps(dict(figure="eager_us_per_call", rows=rows, particles=K, **launch_times(rows, K))), flush=True)


if __name__ == "__main__":
    main()
