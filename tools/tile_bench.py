#!/usr/bin/env python
"""Measurements of tiled scene parsing (attend_infer_repeat_amd/tile.py); prints one JSON line and a readable table.

  parse    the captured TiledSceneParser.parse() over a captured SceneParser at --scenes scenes of --scene pixels, window 50 x 50,
           stride --stride (defaults: 64 scenes of 100 x 100 at stride 25: 9 windows, 576 provider rows), untrained parameters with
           given counts r mod (T + 1) so that every window count occurs.  Beside it the same outputs from public calls: windows by
           torch `unfold`, SceneParser.parse, tile.reference_merge on the host, the existing read-out entries called eagerly.  The two
           routes must agree exactly -- counts, kept_cand, every owner pixel -- or the tool exits with an error.
  gather   air_tile_gather alone at --gather-scenes scenes (default 8192) against a device-to-device copy of the bytes it writes.

Timing: a warm-up, then 5 repeats of --iters calls each between device events; the median repeat is reported with all repeats.  The
two routes of `parse` alternate inside one process."""
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
    return e0.elapsed_time(e1) / iters


def median_ms(fn, iters, stream):
    fn(); fn()
    torch.cuda.synchronize()
    reps = [timed(fn, iters, stream) for _ in range(5)]
    return statistics.median(reps), reps


def public_route(ps, scenes, counts, scene, stride, bufs):
    """the tiled parse from public calls; returns (num_objects [S], kept_cand [C, S] as numpy, owner [S, Hs, Ws] on the device)"""
    from attend_infer_repeat_amd import _lib, hip as H, tile
    cfg = ps.engine.cfg
    (Hi, Wi), (hc, wc), (Hs, Ws) = cfg.img_size, cfg.crop_size, scene
    S = scenes.shape[0]
    windows = scenes.unfold(1, Hi, stride[0]).unfold(2, Wi, stride[1]).reshape(-1, Hi, Wi)       # (the sizes divide: no clamped window)
    base = ps.parse(windows, counts)
    host = lambda t: t.cpu().numpy()
    T = ps.T
    ref = tile.reference_merge(host(base["what"]), host(base["where"]), host(base["glimpse"]).reshape(T, ps.R, -1), host(base["score"]),
                               host(base["num_objects"]), scene, (Hi, Wi), stride)
    C, A = ref["what"].shape[0], ref["what"].shape[2]
    for k in ("what", "where", "glimpse"):
        bufs[k].copy_(torch.from_numpy(ref[k]))
    bufs["n"].copy_(torch.from_numpy(ref["num_objects"]))
    L, p, sp = H.lib(), H._p, H._stream()
    nb = int(L.air_canvas_unroll_bands(S, Hs))
    _lib.check(L.air_parse_objects(None, p(bufs["n"]), p(bufs["where"]), p(bufs["what"]), C, S, A, Hs, Ws, p(bufs["num_objects"]),
                                   p(bufs["count_prob"]), p(bufs["presence"]), p(bufs["score"]), p(bufs["boxes"]), p(bufs["offsets"]),
                                   p(bufs["obj_image"]), p(bufs["obj_step"]), p(bufs["obj_box"]), p(bufs["obj_score"]),
                                   p(bufs["obj_where"]), p(bufs["obj_what"]), sp), "air_parse_objects")
    _lib.check(L.air_parse_render(p(bufs["glimpse"]), p(bufs["where"]), p(bufs["presence"]), p(scenes), float(cfg.output_multiplier),
                                  float(cfg.output_std), ps.mask_threshold, C, S, Hs, Ws, hc, wc, nb, p(bufs["reconstruction"]),
                                  p(bufs["rec_parts"]), p(bufs["owner"]), p(bufs["area"]), None, sp), "air_parse_render")
    _lib.check(L.air_sum_leading(p(bufs["rec_parts"]), p(bufs["rec"]), nb, ctypes.c_size_t(S), sp), "air_sum_leading")
    return ref["num_objects"], ref["kept_cand"], bufs["owner"]


def parse_mode(args, res):
    from attend_infer_repeat_amd import hip as H, tile
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    cfg = EngineConfig()
    S, scene, stride = args.scenes, tuple(args.scene), (args.stride, args.stride)
    _, _, (ny, nx) = tile.check_arguments(cfg, scene, stride, 0.5, S)
    if (scene[0] - cfg.img_size[0]) % stride[0] or (scene[1] - cfg.img_size[1]) % stride[1]:
        raise SystemExit("the public route cuts windows with torch.unfold: (scene - window) must be a multiple of the stride")
    ps = SceneParser(cfg, S * ny * nx, seed=0)
    ps.capture()
    tp = tile.TiledSceneParser(ps, scene, stride)
    tp.capture()
    dev = ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    scenes = (torch.rand(S, *scene, generator=gen) * (torch.rand(S, *scene, generator=gen) > 0.8)).to(dev)
    counts = (torch.arange(ps.R, device=dev) % (ps.T + 1)).to(torch.int32)
    C, A, G = tp.T, int(cfg.n_appearance), cfg.n_crop
    nb = int(H.lib().air_canvas_unroll_bands(S, scene[0]))
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    i32 = torch.int32
    bufs = dict(what=z((C, S, A)), where=z((C, S, 4)), glimpse=z((C, S, G)), n=z((S,), i32), num_objects=z((S,), i32),
                count_prob=z((S,)), presence=z((C, S)), score=z((C, S)), boxes=z((C, S, 4)), offsets=z((S + 1,), i32),
                obj_image=z((C * S,), i32), obj_step=z((C * S,), i32), obj_box=z((C * S, 4)), obj_score=z((C * S,)),
                obj_where=z((C * S, 4)), obj_what=z((C * S, A)), reconstruction=z((S,) + scene), rec_parts=z((nb, S)), rec=z((S,)),
                owner=z((S,) + scene, torch.int8), area=z((C, S), i32))
    stream = torch.cuda.current_stream()
    # agreement first
    out = tp.parse(scenes, counts)
    torch.cuda.synchronize()
    got = {k: out[k].clone() for k in ("num_objects", "kept_cand", "owner", "merge_counts")}
    n_ref, kept_ref, owner_ref = public_route(ps, scenes, counts, scene, stride, bufs)
    torch.cuda.synchronize()
    agree = dict(num_objects=bool((got["num_objects"].cpu().numpy() == n_ref).all()),
                 kept_cand=bool((got["kept_cand"].cpu().numpy() == kept_ref).all()),
                 owner_pixels=bool(torch.equal(got["owner"], owner_ref)))
    res["parse"] = dict(scenes=S, scene=list(scene), stride=list(stride), windows=ny * nx, provider_rows=ps.R, slots=C,
                        agreement=agree, objects_kept=int(n_ref.sum()), merge_counts=got["merge_counts"].sum(0).tolist())
    if not all(agree.values()):
        print(json.dumps(res))
        raise SystemExit("the captured route and the public route disagree: %r" % (agree,))
    provider_ms, provider_reps = median_ms(lambda: ps.parse(tp.windows.view(ps.R, *cfg.img_size), counts), args.iters, stream)
    tiled_ms, tiled_reps = median_ms(lambda: tp.parse(scenes, counts), args.iters, stream)
    public_ms, public_reps = median_ms(lambda: public_route(ps, scenes, counts, scene, stride, bufs), max(args.iters // 4, 2), stream)
    tiled_ms2, tiled_reps2 = median_ms(lambda: tp.parse(scenes, counts), args.iters, stream)
    res["parse"].update(provider_graph_ms=provider_ms, provider_repeats_ms=provider_reps, tiled_graph_ms=tiled_ms,
                        tiled_repeats_ms=tiled_reps, tiled_graph_again_ms=tiled_ms2, tiled_again_repeats_ms=tiled_reps2,
                        public_route_ms=public_ms, public_repeats_ms=public_reps, tiled_added_ms=tiled_ms - provider_ms,
                        scenes_per_s=S / (tiled_ms * 1e-3))
    # every launch of the list, eagerly
    from attend_infer_repeat_amd import _lib
    tp.parse(scenes, counts)
    eng, per = ps.engine, {}
    for _ in range(7):
        for name, seg in tp.segments.items():
            for (fn, a, entry) in seg:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(eng.stream)
                _lib.check(fn(*a, eng._sp()), entry)
                e1.record(eng.stream)
                e1.synchronize()
                per.setdefault(entry, []).append(e0.elapsed_time(e1) * 1e3)
    res["parse"]["eager_launch_us"] = {k: statistics.median(v) for k, v in per.items()}
    tp.release_graphs(); ps.release_graphs()


def gather_mode(args, res):
    from attend_infer_repeat_amd import _lib, hip as H, tile
    S, scene, img, stride = args.gather_scenes, tuple(args.scene), (50, 50), (args.stride, args.stride)
    _, _, (ny, nx) = tile.check_geometry(scene, img, stride, n_scenes=S)
    scenes = torch.rand(S, *scene, device="cuda")
    out = torch.empty(S * ny * nx, img[0] * img[1], device="cuda")
    other = torch.empty_like(out)
    L, p = H.lib(), H._p
    stream = torch.cuda.current_stream()
    gather = lambda: _lib.check(L.air_tile_gather(p(scenes), S, scene[0], scene[1], img[0], img[1], stride[0], stride[1], p(out),
                                                  H._stream()), "air_tile_gather")
    copy = lambda: other.copy_(out)
    g_ms, g_reps = median_ms(gather, args.iters, stream)
    c_ms, c_reps = median_ms(copy, args.iters, stream)
    g2_ms, g2_reps = median_ms(gather, args.iters, stream)
    written, read = out.numel() * 4, scenes.numel() * 4
    res["gather"] = dict(scenes=S, scene=list(scene), windows=ny * nx, bytes_written=written, bytes_read_once=read,
                         gather_ms=g_ms, gather_repeats_ms=g_reps, gather_again_ms=g2_ms, gather_again_repeats_ms=g2_reps,
                         copy_ms=c_ms, copy_repeats_ms=c_reps, gather_write_GBps=written / (g_ms * 1e-3) / 1e9,
                         copy_write_GBps=written / (c_ms * 1e-3) / 1e9)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["parse", "gather"], choices=("parse", "gather"))
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--gather-scenes", type=int, default=8192)
    ap.add_argument("--scene", type=int, nargs=2, default=[100, 100])
    ap.add_argument("--stride", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tile_bench measures on the GPU; there is no CPU fallback")
    res = dict(tool="tile_bench", device=torch.cuda.get_device_name(0))
    if "parse" in args.modes:
        parse_mode(args, res)
    if "gather" in args.modes:
        gather_mode(args, res)
    print(json.dumps(res))
    for mode in ("parse", "gather"):
        for k, v in res.get(mode, {}).items():
            print("%-8s %-28s %s" % (mode, k, v))
    return res


if __name__ == "__main__":
    main()
