#!/usr/bin/env python
"""Measurements of the importance-weighted evaluation (attend_infer_repeat_amd/iw_eval.py); one JSON line per call.

  --point e2e     particles per second of the captured ImportanceEvaluator at --batch x --particles rows, against what the
                  public API offers without it: an eager AIREngine.forward() at the same row count, outputs(), and the same
                  log-weight / logsumexp written in torch on the device (built here from public calls only, never from the
                  new kernels).  Also the launch count of the evaluation graph.
  --point kernel  air_iw_logweight alone at --rows rows (T = 3, A = 50): achieved bytes/s from the algorithmic bytes
                  4 R (T (3A + 12 + 1) + 3), next to a device-to-device copy of the same byte count in the same run.

Timing: a warm-up, then 5 alternating repeats (candidate, baseline, candidate, ...) of --iters calls each; the median repeat is
reported.  The kernel point is timed with device events; the e2e point with the host clock between two device synchronisations,
because the baseline contains host synchronisations of its own (outputs()).  Run each call under its own `timeout`."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def torch_log_weights(eng, K, normalize=True):
    """the evaluator's arithmetic from AIREngine.outputs() in torch (device ops on the current stream)"""
    cfg, T = eng.cfg, eng.T
    o = eng.outputs()
    N = torch.distributions.Normal
    z = o["presence"].reshape(T, -1)
    n = z.sum(0).long()
    lr_what = (N(cfg.what_prior[0], cfg.what_prior[1]).log_prob(o["what"]) - N(o["what_loc"], o["what_scale"]).log_prob(o["what"])).sum(-1)
    wl = o["where_loc"]
    p_loc = torch.zeros_like(wl)
    p_loc[..., 0::2] = cfg.where_scale_prior[0]
    p_loc[..., 1::2] = wl[..., 1::2] if cfg.where_shift_prior[0] is None else cfg.where_shift_prior[0]
    p_scale = torch.tensor([cfg.where_scale_prior[1], cfg.where_shift_prior[1]] * 2, device=wl.device)
    lr_where = (N(p_loc, p_scale).log_prob(o["where"]) - N(wl, o["where_scale"]).log_prob(o["where"])).sum(-1)
    prior = eng.prior_dev / eng.prior_dev.sum() if normalize else eng.prior_dev
    logw = -o["rec_loss_per_sample"] + (torch.log(prior)[n] - o["num_steps_log_prob"].double()).float() + (z * (lr_what + lr_where)).sum(0)
    lw = logw.reshape(-1, K)
    wn = torch.softmax(lw, 1)
    q = torch.stack([(wn * (n.reshape(-1, K) == c)).sum(1) for c in range(T + 1)], 1)
    return dict(iw_bound=torch.logsumexp(lw, 1) - math.log(K), elbo=lw.mean(1), ess=1.0 / (wn * wn).sum(1), q=q, logw=lw)


def alternate(candidates, iters, repeats=5):
    """median seconds per call of each candidate over `repeats` alternating rounds"""
    times = {k: [] for k in candidates}
    for k, fn in candidates.items():
        fn()                                                     # warm-up
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in candidates.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters)
    return {k: statistics.median(v) for k, v in times.items()}, times


def point_e2e(args):
    from attend_infer_repeat_amd.engine import AIREngine, EngineConfig
    from attend_infer_repeat_amd.iw_eval import ImportanceEvaluator
    B, K = args.batch, args.particles
    cfg = EngineConfig(mfma_dtype=args.mfma)
    ev = ImportanceEvaluator(cfg, B, K, seed=0)
    ev.set_global_step(20000)
    ev.capture()
    base = AIREngine(cfg, B * K, seed=0)                           # what a user has today: the training configuration, eager forward
    base.load_parameters({k: v for k, v in ev.engine.params.items()})
    base.set_global_step(20000)
    obs = torch.rand(B, *cfg.img_size, device="cuda")
    tiled = obs.repeat_interleave(K, 0)

    def run_evaluator():
        ev.evaluate(obs)

    def run_public():
        base.forward(tiled, sample_noise=True)
        out = torch_log_weights(base, K)
        base.wait_for_caller()
        return out

    med, raw = alternate({"evaluator": run_evaluator, "public_calls": run_public}, args.iters)
    # the two compute the same thing (own noise streams, so compare the batch mean of the bound loosely)
    a = ev.evaluate(obs)["iw_bound"].double().mean().item()
    b = run_public()["iw_bound"].double().mean().item()
    lc = ev.launch_count()
    return dict(point="e2e", batch=B, particles=K, rows=B * K, mfma=args.mfma, iters=args.iters,
                evaluator_ms=med["evaluator"] * 1e3, public_calls_ms=med["public_calls"] * 1e3,
                evaluator_particles_per_s=B * K / med["evaluator"], public_calls_particles_per_s=B * K / med["public_calls"],
                speedup=med["public_calls"] / med["evaluator"], repeats_ms={k: [x * 1e3 for x in v] for k, v in raw.items()},
                graph_entries=lc, graph_entries_total=sum(lc.values()), mean_iw_bound=dict(evaluator=a, public_calls=b))


def point_kernel(args):
    from attend_infer_repeat_amd import _lib, hip as H
    R, T, A, K = args.rows, 3, 50, 64
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    what, what_loc, what_scale = rn(T, R, A), rn(T, R, A), rn(T, R, A).abs() + 0.1
    where, where_loc, where_scale = rn(T, R, 4), rn(T, R, 4), rn(T, R, 4).abs() + 0.1
    rec, logp = rn(R), -rn(R).abs()
    prior = torch.tensor([0.4, 0.3, 0.2, 0.1], dtype=torch.float64, device=dev)
    logw, n = torch.zeros(R, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    p, L = H._p, H.lib()
    nbytes = 4 * R * (T * (3 * A + 12 + 1) + 3)
    src, dst = torch.empty(nbytes // 4, device=dev), torch.empty(nbytes // 4, device=dev)
    src.normal_(generator=g)
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters

    out = {}
    for tag, presence in (("all_steps_present", torch.ones(T, R, device=dev)),
                          ("mixed_counts", (torch.arange(T, device=dev)[:, None] < torch.randint(0, T + 1, (R,), device=dev, generator=g)[None]).float())):
        def kernel():
            _lib.check(L.air_iw_logweight(p(what), p(what_loc), p(what_scale), p(where), p(where_loc), p(where_scale), p(presence), p(rec),
                                          p(logp), p(prior), T, R, K, A, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1, p(logw), p(n), sp), "air_iw_logweight")
        copy = lambda: dst.copy_(src)
        kernel(); copy()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(5):
            tk.append(timed(kernel, args.iters)); tc.append(timed(copy, args.iters))
        k_med, c_med = statistics.median(tk), statistics.median(tc)
        out[tag] = dict(kernel_us=k_med * 1e6, copy_us=c_med * 1e6, kernel_over_copy=k_med / c_med,
                        kernel_algorithmic_GBps=nbytes / k_med * 1e-9, copy_GBps_read=nbytes / c_med * 1e-9,
                        copy_GBps_read_plus_write=2 * nbytes / c_med * 1e-9, finite=bool(torch.isfinite(logw).all().item()))
    return dict(point="kernel", rows=R, T=T, A=A, algorithmic_bytes=nbytes, iters=args.iters, **out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=("e2e", "kernel"), required=True)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--particles", type=int, default=16)
    ap.add_argument("--mfma", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args(argv)
    res = point_e2e(args) if args.point == "e2e" else point_kernel(args)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
