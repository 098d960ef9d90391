#!/usr/bin/env python
"""Measurements of parse scoring (attend_infer_repeat_amd/score.py); one JSON line per call.

  --point e2e          the captured ParseScorer.score() at --images images next to the same outputs from torch on the device (the
                       route a user has without the kernels: bincount of owner * (G + 1) + gt per image, float64 box and mask IoU,
                       a Python greedy loop over thresholds and steps, ARI from the table, the sums), and the time of each of the three
                       launches issued eagerly.  Owner maps and boxes come from a real parse of annotated glyph canvases (given
                       counts = the true ones: an untrained model's own mode is n = 0 everywhere); 1024 distinct canvases, tiled.
  --point contingency  air_score_contingency alone at --images images (the parse's owner maps, tiled) next to a device-to-device
                       copy of its minimal byte count, 2 R H W (the two int8 maps read once; the table is negligible).
  --shape c1 | c4      50x50, T = 3, G = 2  |  100x100, T = 5, G = 4

Timing: a warm-up, then 5 repeats of --iters calls each (the contingency point alternates kernel and copy); the median repeat is
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {"c1": dict(img_size=(50, 50), crop_size=(20, 20), max_steps=3, G=2),
          "c4": dict(img_size=(100, 100), crop_size=(28, 28), max_steps=5, G=4)}
DISTINCT = 1024


def timed(fn, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def parsed_glyphs(shape, R):
    """a SceneParser at R images holding the parse of annotated glyph canvases, and the annotations on the device"""
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.parse import SceneParser
    s = SHAPES[shape]
    G = s["G"]
    d = procedural_multi_mnist(min(R, DISTINCT), canvas_size=s["img_size"], n_objects=(0, G), seed=0, n_templates=1000,
                               return_annotations=True)
    reps = -(-R // d["imgs"].shape[0])
    tile = lambda a: torch.from_numpy(np.concatenate([a] * reps, 0)[:R]).cuda()
    obs, inst, boxes = tile(d["imgs"].astype(np.float32) / 255.0), tile(d["instances"]), tile(d["boxes"])
    counts = (boxes[:, :, 2] > 0).sum(1).int()
    ps = SceneParser(EngineConfig(img_size=s["img_size"], crop_size=s["crop_size"], max_steps=s["max_steps"]), R, seed=0)
    ps.capture()
    ps.parse(obs, counts)
    ps.synchronize()
    return ps, inst, boxes, counts


def torch_route(owner, boxes, num_objects, score, gt, gt_boxes, gt_count, thresholds, T, G):
    """the scorer's outputs from torch ops on the device (host-side control flow)"""
    R = owner.shape[0]
    nb = (T + 1) * (G + 1)
    code = (owner.long() + 1) * (G + 1) + (gt.long() + 1)
    code = code.reshape(R, -1) + torch.arange(R, device=owner.device)[:, None] * nb
    cont = torch.bincount(code.reshape(-1), minlength=R * nb).reshape(R, T + 1, G + 1)
    nh, g = num_objects.long().clamp(0, T), gt_count.long().clamp(0, G)
    live = (torch.arange(T, device=owner.device)[None, :, None] < nh[:, None, None]) & \
           (torch.arange(G, device=owner.device)[None, None, :] < g[:, None, None])
    a, b = boxes.permute(1, 0, 2).double()[:, :, None, :], gt_boxes.double()[:, None, :, :]      # [R,T,1,4], [R,1,G,4]
    lo = lambda x, i: torch.minimum(x[..., i], x[..., i] + x[..., i + 2])
    hi = lambda x, i: torch.maximum(x[..., i], x[..., i] + x[..., i + 2])
    iw = (torch.minimum(hi(a, 0), hi(b, 0)) - torch.maximum(lo(a, 0), lo(b, 0))).clamp_min(0)
    ih = (torch.minimum(hi(a, 1), hi(b, 1)) - torch.maximum(lo(a, 1), lo(b, 1))).clamp_min(0)
    inter = iw * ih
    union = (hi(a, 0) - lo(a, 0)) * (hi(a, 1) - lo(a, 1)) + (hi(b, 0) - lo(b, 0)) * (hi(b, 1) - lo(b, 1)) - inter
    q = inter / union
    box_iou = torch.where((inter > 0) & (union > 0) & torch.isfinite(q) & live, q, torch.zeros_like(q))
    n = cont[:, 1:, 1:].double()
    mu = cont[:, 1:].sum(2).double()[:, :, None] + cont[:, :, 1:].sum(1).double()[:, None, :] - n
    mask_iou = torch.where((mu > 0) & live, n / mu.clamp_min(1), torch.zeros_like(n))
    match = []
    for tau in thresholds:
        used = torch.zeros(R, G, dtype=torch.bool, device=owner.device)
        rows = []
        for t in range(T):
            v = box_iou[:, t]
            cand = torch.where((v > 0) & (v >= float(np.float32(tau))) & ~used, v, torch.full_like(v, -1.0))
            top, j = cand.max(1)                                   # the first maximal index
            pick = torch.where(top > 0, j, torch.full_like(j, -1))
            used |= torch.nn.functional.one_hot(pick.clamp_min(0), G).bool() & (pick >= 0)[:, None]
            rows.append(pick)
        match.append(torch.stack(rows, 0))
    match = torch.stack(match, 0)                                  # [K,T,R]
    fg = cont[:, :, 1:]
    pairs = lambda x: x * (x - 1) // 2
    N, S = fg.sum((1, 2)), pairs(fg).sum((1, 2))
    P, Q, C = pairs(fg.sum(2)).sum(1).double(), pairs(fg.sum(1)).sum(1).double(), pairs(N).double()
    E, M = P * Q / C, (P + Q) / 2
    ari = torch.where(N == 0, torch.full_like(E, float("nan")), torch.where((C == 0) | (M == E), torch.ones_like(E), (S - E) / (M - E)))
    best = torch.where(torch.arange(G, device=owner.device)[None] < g[:, None], mask_iou.max(1).values, -torch.ones_like(mask_iou[:, 0]))
    err = nh - g
    fin = torch.isfinite(ari)
    tp = (match >= 0).sum((1, 2))
    m0 = match[0].t()                                              # [R,T]
    totals_i = torch.cat([torch.stack([torch.tensor(R, device=owner.device), (err == 0).sum(), err.abs().sum(), nh.sum(), g.sum(),
                                       fin.sum()]), tp])
    totals_f = torch.stack([ari[fin].sum(), best.clamp_min(0).sum(),
                            (box_iou.gather(2, m0.clamp_min(0)[:, :, None])[:, :, 0] * (m0 >= 0)).sum()])
    return dict(cont=cont.int(), box_iou=box_iou.float(), mask_iou=mask_iou.float(), match=match.to(torch.int8), ari=ari.float(),
                best_overlap=best.float(), count_err=err.int(), totals_i=totals_i, totals_f=totals_f)


def point_e2e(args):
    from attend_infer_repeat_amd import _lib
    from attend_infer_repeat_amd.score import ParseScorer
    R, G = args.images, SHAPES[args.shape]["G"]
    ps, inst, boxes, counts = parsed_glyphs(args.shape, R)
    sc = ParseScorer(ps, G)
    sc.capture()
    stream = torch.cuda.current_stream()
    call = lambda: sc.score(inst, boxes, counts, accumulate=False)
    call(); call()
    torch.cuda.synchronize()
    reps = [timed(call, args.iters, stream) for _ in range(5)]
    out = {k: v.clone() for k, v in call().items()}
    summary = sc.summary()
    eng, sp, per = ps.engine, ps.engine._sp(), {}
    for _ in range(5):
        for i, (fn, a, name) in enumerate(sc._plans[False]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, sp), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault("%02d %s" % (i, name), []).append(e0.elapsed_time(e1) * 1e3)
    route = lambda: torch_route(ps.owner, ps.boxes, ps.num_objects, ps.score, inst, boxes, counts, sc.thresholds_host, ps.T, G)
    ref = route(); route()
    torch.cuda.synchronize()
    iters_t = max(args.iters // 4, 2)
    reps_t = [timed(route, iters_t, stream) for _ in range(5)]
    agree = {k: bool(torch.equal(ref[k], out[k])) for k in ("cont", "match", "count_err", "totals_i")}
    agree.update({k + "_max_abs_diff": float((ref[k].double() - out[k].double()).abs().nan_to_num(0).max().item())
                  for k in ("box_iou", "mask_iou", "ari", "best_overlap", "totals_f")})
    med = statistics.median(reps)
    return dict(point="e2e", shape=args.shape, images=R, iters=args.iters, score_graph_us=med * 1e6, images_per_s=R / med,
                repeats_us=[x * 1e6 for x in reps], torch_route_us=statistics.median(reps_t) * 1e6,
                torch_repeats_us=[x * 1e6 for x in reps_t], eager_launch_us={k: statistics.median(v) for k, v in per.items()},
                owned_pixel_share=float((ps.owner >= 0).double().mean().item()), agree=agree,
                summary={k: summary[k] for k in ("count_acc", "map", "fg_ari", "mean_best_overlap", "matched_box_iou")})


def point_contingency(args):
    from attend_infer_repeat_amd import _lib, hip as H
    s = SHAPES[args.shape]
    R, T, G, (Hi, Wi) = args.images, s["max_steps"], s["G"], s["img_size"]
    ps, inst, _, _ = parsed_glyphs(args.shape, min(R, DISTINCT))
    reps = -(-R // inst.shape[0])
    owner, gt = ps.owner.repeat(reps, 1, 1)[:R].contiguous(), inst.repeat(reps, 1, 1)[:R].contiguous()
    cont = torch.empty(R, T + 1, G + 1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    L, p = H.lib(), H._p
    nbytes = 2 * R * Hi * Wi
    src, dst = torch.empty(nbytes // 2, dtype=torch.int8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.int8, device="cuda")
    kernel = lambda: _lib.check(L.air_score_contingency(p(owner), p(gt), T, G, R, Hi, Wi, p(cont), sp), "air_score_contingency")
    copy = lambda: dst.copy_(src)
    kernel(); copy()
    torch.cuda.synchronize()
    tk, tc = [], []
    for _ in range(5):
        tk.append(timed(kernel, args.iters, stream)); tc.append(timed(copy, args.iters, stream))
    k_med, c_med = statistics.median(tk), statistics.median(tc)
    return dict(point="contingency", shape=args.shape, images=R, iters=args.iters, minimal_bytes=nbytes, kernel_us=k_med * 1e6,
                copy_us=c_med * 1e6, kernel_GBps=nbytes / k_med * 1e-9, copy_GBps_read_plus_write=nbytes / c_med * 1e-9,
                kernel_over_copy_bandwidth=c_med / k_med, pixels_per_s=R * Hi * Wi / k_med, kernel_repeats_us=[x * 1e6 for x in tk],
                owned_pixel_share=float((owner >= 0).double().mean().item()), pixels_counted=int(cont.sum().item()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=("e2e", "contingency"), required=True)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c1")
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    res = point_e2e(args) if args.point == "e2e" else point_contingency(args)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
