#!/usr/bin/env python
"""Measurements of scene generation (attend_infer_repeat_amd/generate.py) at the configs[1] shapes (50x50 / 20x20 / T = 3);
one JSON line per call.

  --point e2e      scenes per second of the captured SceneSampler at --scenes scenes (one hipGraph replay per call), and the time
                   of every launch of the same chain issued eagerly, from device events around each entry.
  --point observe  air_observe alone on --scenes x 2500 pixels: achieved bytes/s on its minimal traffic -- 4n read plus 8n (mean and
                   obs) or 4n (obs alone) written -- with and without the pixel noise, next to a device-to-device copy of the same
                   byte count timed in the same process.

Timing: a warm-up, then 5 repeats of --iters calls each (the observe point alternates kernel and copy); the median repeat is
reported.  Device events throughout.  Run each call under its own `timeout`."""
import argparse
import ctypes
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


def point_e2e(args):
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.generate import SceneSampler
    R = args.scenes
    s = SceneSampler(EngineConfig(mfma_dtype=args.mfma), R, seed=0, count_probs="uniform")
    s.capture()
    stream = torch.cuda.current_stream()
    s.sample(); s.sample()
    torch.cuda.synchronize()
    reps = [timed(s.sample, args.iters, stream) for _ in range(5)]
    med = statistics.median(reps)
    # per launch: the same entries issued one by one on the sampler's stream, an event pair around each
    plan, sp = s._plans[(True, False)], s._sp()
    per = {}
    for _ in range(3):
        for i, (fn, a, name) in enumerate(plan):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s.stream)
            _lib.check(fn(*a, sp), name)
            e1.record(s.stream)
            e1.synchronize()
            per.setdefault("%02d %s" % (i, name), []).append(e0.elapsed_time(e1) * 1e3)
    out = s.sample()
    hist = torch.bincount(out["num_objects"].long(), minlength=s.T + 1).tolist()
    return dict(point="e2e", scenes=R, mfma=args.mfma, iters=args.iters, graph_ms=med * 1e3, scenes_per_s=R / med,
                repeats_ms=[x * 1e3 for x in reps], launches=sum(s.launch_count().values()),
                eager_launch_us={k: statistics.median(v) for k, v in per.items()}, count_hist=hist,
                finite=bool(torch.isfinite(out["obs"]).all().item()))


def point_observe(args):
    from attend_infer_repeat_amd import _lib, hip as H
    n = args.scenes * 2500
    dev = "cuda"
    canvas = torch.rand(n, device=dev)
    mean, obs = torch.empty(n, device=dev), torch.empty(n, device=dev)
    state = torch.tensor([0, 0], dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    L, p = H.lib(), H._p
    nan = float("nan")
    out = {}
    for tag, std, want_mean in (("noise_mean_and_obs", 0.3, True), ("noise_obs_only", 0.3, False), ("no_noise_mean_and_obs", 0.0, True),
                                ("no_noise_obs_only", 0.0, False)):
        nbytes = 4 * n * (3 if want_mean else 2)
        src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)      # a copy moves its bytes twice
        src.normal_()

        def kernel():
            _lib.check(L.air_observe(p(canvas), 0.5, std, p(state), 0, nan, nan, p(mean) if want_mean else None, p(obs), n, sp), "air_observe")
        copy = lambda: dst.copy_(src)
        kernel(); copy()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(5):
            tk.append(timed(kernel, args.iters, stream)); tc.append(timed(copy, args.iters, stream))
        k_med, c_med = statistics.median(tk), statistics.median(tc)
        out[tag] = dict(kernel_us=k_med * 1e6, copy_us=c_med * 1e6, minimal_bytes=nbytes, kernel_GBps=nbytes / k_med * 1e-9,
                        copy_GBps_read_plus_write=nbytes / c_med * 1e-9, kernel_over_copy_bandwidth=c_med / k_med,
                        pixels_per_s=n / k_med, finite=bool(torch.isfinite(obs).all().item()))
        del src, dst
    return dict(point="observe", scenes=args.scenes, pixels=n, iters=args.iters, **out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=("e2e", "observe"), required=True)
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--mfma", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args(argv)
    res = point_e2e(args) if args.point == "e2e" else point_observe(args)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
