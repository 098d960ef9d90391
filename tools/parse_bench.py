#!/usr/bin/env python
"""Measurements of scene parsing (attend_infer_repeat_amd/parse.py) at the configs[1] shapes (50x50 / 20x20 / T = 3, A = 50);
one JSON line per call.

  --point e2e     the captured SceneParser.parse() at --images images (one hipGraph replay per call) next to
                  (a) the same outputs from public calls: eager AIREngine.forward(sample_noise=False) at noise 0 / 0 / -1, outputs(),
                      and torch for the count (float64 chain + argmax), the boxes, the per-step hip.st_write_fwd, the running sum,
                      the arg-max with its threshold, the areas and the object table;
                  (b) the forward plan alone, captured as a graph of its own: the difference to the parse is what the read-out
                      entries cost;
                  --counts cycle (default) gives the counts r mod (T + 1) to both routes, --counts model takes the mode of q(n | x);
                  and the time of every launch of the parse chain issued eagerly (device events around each entry).
  --point render  air_parse_render alone at --images images (random glimpses, boxes inside the canvas, counts r mod (T + 1) or all
                  T with --all-present) next to a device-to-device copy of its minimal byte count:
                  4 (T hw + 4 T + T) read per image + 4 HW of obs, 5 HW written (reconstruction fp32 + owner int8).

Timing: a warm-up, then 5 repeats of --iters calls each (the render point alternates kernel and copy); the median repeat is
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


def public_route(eng, obs, thr, given=None):
    """the parser's outputs from public calls + torch (host-side control flow, device tensors)"""
    from attend_infer_repeat_amd import hip as H
    cfg, T, R = eng.cfg, eng.T, eng.B
    (Hi, Wi) = cfg.img_size
    eng.forward(obs, sample_noise=False)
    o = eng.outputs()
    eng.wait_for_engine()
    p = o["presence_prob"].reshape(T, R).double()
    cum = torch.cumprod(p, 0)
    m = torch.cat([(1 - p[:1]), (1 - p[1:]) * cum[:-1], cum[-1:]], 0)                       # [T + 1, R]
    q = m / m.sum(0, keepdim=True)
    n = m.argmax(0) if given is None else given.long().clamp(0, T)                          # (argmax: the first maximal index)
    count_prob = q.gather(0, n[None]).float()[0]
    score = q.flip(0).cumsum(0).flip(0)[1:].float()
    presence = (torch.arange(T, device=p.device)[:, None] < n[None, :]).float()
    w = o["where"]
    boxes = torch.stack([Wi * (1 - w[..., 0] + w[..., 1]) / 2, Hi * (1 - w[..., 2] + w[..., 3]) / 2, Wi * w[..., 0], Hi * w[..., 2]], -1)
    glimpse = o["glimpse_raw"].reshape(T, R, *cfg.crop_size)
    layers = torch.stack([H.st_write_fwd(glimpse[t], w[t], cfg.img_size) for t in range(T)], 0) * cfg.output_multiplier
    masked = torch.where(presence[:, :, None, None] > 0.5, layers, torch.full_like(layers, float("-inf")))
    top, arg = masked.max(0)
    owner = torch.where(top > thr, arg, torch.full_like(arg, -1)).to(torch.int8)
    rec_img = (layers * presence[:, :, None, None]).sum(0)
    z = (obs.reshape(R, Hi, Wi) - rec_img) / cfg.output_std
    rec = (0.5 * z * z).reshape(R, -1).sum(1)
    area = torch.stack([(owner == t).reshape(R, -1).sum(1) for t in range(T)], 0).int()
    offsets = torch.cat([n.new_zeros(1), n.cumsum(0)]).int()
    r_idx, t_idx = presence.t().nonzero(as_tuple=True)
    table = (r_idx.int(), t_idx.int(), boxes[t_idx, r_idx], score[t_idx, r_idx], w[t_idx, r_idx], o["what"][t_idx, r_idx])
    return dict(num_objects=n.int(), count_prob=count_prob, score=score, presence=presence, boxes=boxes, owner=owner,
                reconstruction=rec_img, rec=rec, area=area, offsets=offsets, table=table)


def point_e2e(args):
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.engine import AIREngine
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.iw_eval import inner_config
    from attend_infer_repeat_amd.parse import SceneParser
    R = args.images
    cfg = EngineConfig(mfma_dtype=args.mfma)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    eng = ps.engine
    obs = torch.rand(R, *cfg.img_size, device=eng.device)
    stream = torch.cuda.current_stream()
    given = None if args.counts == "model" else (torch.arange(R, device=eng.device) % (ps.T + 1)).int()
    call = lambda: ps.parse(obs, given)
    call(); call()
    torch.cuda.synchronize()
    reps = [timed(call, args.iters, stream) for _ in range(5)]
    med = statistics.median(reps)
    out = ps.parse(obs, given)
    hist = torch.bincount(out["num_objects"].long(), minlength=ps.T + 1).tolist()
    # (b) the forward plan alone, one graph
    g_fwd = eng._capture_plans([list(eng._plan_fwd)])

    def fwd_only():
        eng.wait_for_caller()
        eng._replay_or_run(g_fwd, eng._plan_fwd)
        eng.wait_for_engine()
    fwd_only(); fwd_only()
    torch.cuda.synchronize()
    reps_f = [timed(fwd_only, args.iters, stream) for _ in range(5)]
    # per launch, eagerly
    plan, sp = ps._plans[given is not None], eng._sp()
    per = {}
    for _ in range(3):
        for i, (fn, a, name) in enumerate(plan):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, sp), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault("%02d %s" % (i, name), []).append(e0.elapsed_time(e1) * 1e3)
    # (a) the public-call route on an engine of its own with the same parameters
    pub = AIREngine(inner_config(cfg), R, seed=0, keep_canvas_steps=False)
    pub._sync_param_shadow()                                 # (bf16: see SceneParser.__init__)
    pub.set_noise(torch.zeros_like(pub.eps_where), torch.zeros_like(pub.eps_what), torch.full_like(pub.u_pres, -1.0))
    route = lambda: public_route(pub, obs, ps.mask_threshold, given)
    ref = route(); route()
    torch.cuda.synchronize()
    iters_p = max(args.iters // 2, 2)
    reps_p = [timed(route, iters_p, stream) for _ in range(5)]
    agree = dict(num_objects=bool(torch.equal(ref["num_objects"], out["num_objects"])),
                 owner_mismatch_share=float((ref["owner"] != out["owner"]).double().mean().item()),
                 reconstruction_max_abs_diff=float((ref["reconstruction"] - out["reconstruction"]).abs().max().item()))
    return dict(point="e2e", images=R, mfma=args.mfma, counts=args.counts, iters=args.iters, parse_graph_ms=med * 1e3, images_per_s=R / med,
                repeats_ms=[x * 1e3 for x in reps], forward_graph_ms=statistics.median(reps_f) * 1e3,
                forward_repeats_ms=[x * 1e3 for x in reps_f], public_route_ms=statistics.median(reps_p) * 1e3,
                public_repeats_ms=[x * 1e3 for x in reps_p], launches=ps.launch_count(),
                eager_launch_us={k: statistics.median(v) for k, v in per.items()}, count_hist=hist, agree=agree)


def point_render(args):
    from attend_infer_repeat_amd import _lib, hip as H
    R, T, (Hi, Wi), (hc, wc) = args.images, 3, (50, 50), (20, 20)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    glimpse = torch.randn(T, R, hc, wc, device=dev, generator=g)
    where = torch.empty(T, R, 4, device=dev)
    where[..., 0::2] = 0.3 + 0.4 * torch.rand(T, R, 2, device=dev, generator=g)           # scales 0.3 .. 0.7
    where[..., 1::2] = -0.3 + 0.6 * torch.rand(T, R, 2, device=dev, generator=g)          # shifts: the box stays on the canvas
    n = torch.full((R,), T, device=dev) if args.all_present else torch.arange(R, device=dev) % (T + 1)
    presence = (torch.arange(T, device=dev)[:, None] < n[None, :]).float().contiguous()
    obs = torch.rand(R, Hi, Wi, device=dev, generator=g)
    L, p = H.lib(), H._p
    nb = int(L.air_canvas_unroll_bands(R, Hi))
    recon, rec_parts = torch.empty(R, Hi, Wi, device=dev), torch.empty(nb, R, device=dev)
    owner, area = torch.empty(R, Hi, Wi, dtype=torch.int8, device=dev), torch.empty(T, R, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    nbytes = R * (4 * (T * hc * wc + 4 * T + T) + 4 * Hi * Wi + 5 * Hi * Wi)
    src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)          # a copy moves its bytes twice
    src.normal_()
    out = {}
    for tag, with_obs in (("with_rec", True), ("without_rec", False)):
        def kernel():
            _lib.check(L.air_parse_render(p(glimpse), p(where), p(presence), p(obs) if with_obs else None, 0.5, 0.3, 0.02, T, R, Hi, Wi,
                                          hc, wc, nb, p(recon), p(rec_parts) if with_obs else None, p(owner), p(area), None, sp),
                       "air_parse_render")
        copy = lambda: dst.copy_(src)
        kernel(); copy()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(5):
            tk.append(timed(kernel, args.iters, stream)); tc.append(timed(copy, args.iters, stream))
        k_med, c_med = statistics.median(tk), statistics.median(tc)
        out[tag] = dict(kernel_us=k_med * 1e6, copy_us=c_med * 1e6, kernel_GBps=nbytes / k_med * 1e-9,
                        copy_GBps_read_plus_write=nbytes / c_med * 1e-9, kernel_over_copy_bandwidth=c_med / k_med,
                        pixels_per_s=R * Hi * Wi / k_med, kernel_repeats_us=[x * 1e6 for x in tk])
    owned = float((owner >= 0).double().mean().item())
    return dict(point="render", images=R, bands=nb, all_present=bool(args.all_present), iters=args.iters, minimal_bytes=nbytes,
                owned_pixel_share=owned, area_total=int(area.sum().item()), **out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=("e2e", "render"), required=True)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--mfma", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--all-present", action="store_true")
    ap.add_argument("--counts", default="cycle", choices=("cycle", "model"),
                    help="e2e: 'cycle' parses with given counts r mod (T + 1) (an untrained model's own mode is n = 0 everywhere: "
                         "nothing to render), 'model' with the mode of q(n | x)")
    args = ap.parse_args(argv)
    res = point_e2e(args) if args.point == "e2e" else point_render(args)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
