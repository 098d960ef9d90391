#!/usr/bin/env python
"""Measurements of the temporal proposals (attend_infer_repeat_amd/temporal.py); prints one JSON line and a readable table.

At the tracker benchmark's shapes -- --rows provider rows (default 1024) of 50 x 50 frames, T = 3, --frames F per sequence (default 8):
a captured SceneParser with untrained parameters and given counts r mod (T + 1), so that every frame count occurs and neighbours hold
objects a frame lacks, a captured TemporalProposer over it (--proposals P, --rounds), and on the same rows a captured ParseProposer
with the same P and rounds.  The frames of a sequence are one sparse random image shifted a pixel per frame.

  agreement  every round's pool against temporal.reference_pool on the read-back of the round's input rows: exact, or the tool exits
             with an error;
  provider   the provider's own captured parse() of the R rows;
  temporal   the TemporalProposer's graph alone (all rounds and the read-out), and every round as a graph of its own;
  residual   the ParseProposer's graph alone on the same rows (its rounds run the forward plan on the residual), per round from its
             total minus the read-out;
  and every entry of a temporal round launched eagerly on its own: the share of air_temporal_pool and of air_prune_score.

Timing: a warm-up, then 5 repeats of --iters calls each between device events; the median repeat is reported with all repeats."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def check_pools(tp, base, table, img):
    """every round's pool against the host reference, fed with the device's own round inputs"""
    from attend_infer_repeat_amd import temporal
    host = lambda t: t.detach().cpu().numpy()
    T, R = tp.T, tp.R
    cur = dict(what=host(base["what"]), where=host(base["where"]), glimpse=host(base["glimpse"]).reshape(T, R, -1), score=host(base["score"]))
    n, src = host(base["num_objects"]), None
    agree, states = {}, np.zeros(6, np.int64)
    for r in range(tp.rounds):
        ref = temporal.reference_pool(cur["what"], cur["where"], cur["glimpse"], cur["score"], n, table, tp.F, img, tp.proposals,
                                      tp.iou_novel, tp.direction == "both", tp.interpolate, round=r, source_in=src)
        got = dict(what=tp.pool_what[r], where=tp.pool_where[r], glimpse=tp.pool_glimpse[r], score=tp.pool_score[r],
                   presence=tp.pool_presence[r], source=tp.pool_source[r], cand_state=tp.cand_state[r], taken=tp.proposals_taken[r],
                   partner=tp.partner[r])
        for k, v in got.items():
            a, b = host(v), np.ascontiguousarray(ref[k])
            same = np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)
            agree["round%d_%s" % (r, k)] = bool(same)
        states += np.bincount(ref["cand_state"].reshape(-1), minlength=6)
        cur = {k: host(getattr(tp, "out_" + k)[r, :T]) for k in cur}
        n, src = host(tp.num_objects_round[r]), host(tp.source_out[r])
    return agree, states


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--proposals", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench measures on the GPU; there is no CPU fallback")
    from attend_infer_repeat_amd import _lib, temporal
    from attend_infer_repeat_amd.engine_config import EngineConfig
    from attend_infer_repeat_amd.launch import destroy_graphs
    from attend_infer_repeat_amd.parse import SceneParser
    from attend_infer_repeat_amd.propose import ParseProposer
    cfg = EngineConfig()
    R, F, P, Rn = args.rows, args.frames, args.proposals, args.rounds
    if R % F:
        raise SystemExit("--rows %d is no multiple of %d frames" % (R, F))
    S, T = R // F, int(cfg.max_steps)
    ps = SceneParser(cfg, R, seed=0)
    ps.capture()
    tp = temporal.TemporalProposer(ps, F, P, Rn)
    tp.capture()
    pp = ParseProposer(ps, P, Rn)
    pp.proposal.load_from(ps.engine)                               # the proposal pass runs the provider's parameters
    pp.capture()
    eng, dev = ps.engine, ps.engine.device
    gen = torch.Generator(device="cpu").manual_seed(0)
    start = torch.rand(S, *cfg.img_size, generator=gen) * (torch.rand(S, *cfg.img_size, generator=gen) > 0.8)
    rows_in = torch.stack([torch.roll(start, shifts=(f, f // 2), dims=(1, 2)) for f in range(F)], 1).reshape(R, *cfg.img_size).contiguous().to(dev)
    counts = (torch.arange(R, device=dev) % (T + 1)).to(torch.int32)
    stream = torch.cuda.current_stream()
    base = {k: v.clone() for k, v in ps.parse(rows_in, counts).items()}
    out = tp.parse(rows_in, counts)
    torch.cuda.synchronize()
    agree, states = check_pools(tp, base, tp.engine.prior_dev.cpu().numpy(), tuple(cfg.img_size))
    obj = out["objective_rounds"].cpu().numpy()
    res = dict(tool="temporal_bench", device=torch.cuda.get_device_name(0), frames=F, sequences=S, rows=R, max_steps=T, proposals=P,
               rounds=Rn, agreement_all=all(agree.values()), cand_states=dict(zip(temporal.STATES, states.tolist())),
               proposals_taken=int(out["proposals_taken"].sum()), objects_temporal_kept=int(out["objects_temporal_kept"].sum()),
               objective_never_decreases=bool((obj[1:] >= obj[:-1]).all()))
    if not all(agree.values()):
        print(json.dumps(dict(res, agreement=agree)))
        raise SystemExit("air_temporal_pool and the host reference disagree: %r" % ([k for k, v in agree.items() if not v],))
    provider_ms, provider_reps = median_ms(lambda: ps.parse(rows_in, counts), args.iters, stream)
    total_ms, total_reps = median_ms(lambda: eng._replay_or_run(tp._graph, tp._plan), args.iters, eng.stream)
    round_ms = []
    for r in range(Rn):
        plan = [e for name in temporal.SEGMENTS for e in tp.segments[r][name]]
        eng.synchronize()
        graph = eng._capture_plans([plan])
        round_ms.append(median_ms(lambda: eng._replay_or_run(graph, plan), args.iters, eng.stream))
        destroy_graphs([graph])
    readout_ms, readout_reps = median_ms(lambda: eng._replay_or_run(None, tp.readout), args.iters, eng.stream)
    pp.parse(rows_in, counts)
    torch.cuda.synchronize()
    residual_ms, residual_reps = median_ms(lambda: eng._replay_or_run(pp._graph, pp._plan), args.iters, eng.stream)
    parse_again_ms, _ = median_ms(lambda: tp.parse(rows_in, counts), args.iters, stream)
    per = {}
    plan0 = [e for name in temporal.SEGMENTS for e in tp.segments[0][name]]
    for _ in range(7):
        for (fn, a, name) in plan0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            _lib.check(fn(*a, eng._sp()), name)
            e1.record(eng.stream)
            e1.synchronize()
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    eager = {k: statistics.median(v) for k, v in per.items()}
    eager_round = sum(eager.values())
    temporal_round = statistics.mean(m for m, _ in round_ms)
    residual_round = (residual_ms - readout_ms) / Rn
    A, G = int(cfg.n_appearance), int(cfg.n_crop)
    pool_bytes = R * 4 * ((2 * T + P) * (A + G + 5) + 2 * T * (A + 5))      # read T rows + the candidates' what / where, write C rows
    res.update(provider_graph_ms=provider_ms, provider_repeats_ms=provider_reps, temporal_graph_ms=total_ms, temporal_repeats_ms=total_reps,
               temporal_round_graph_ms=[m for m, _ in round_ms], temporal_round_repeats_ms=[r for _, r in round_ms],
               readout_eager_ms=readout_ms, readout_repeats_ms=readout_reps, residual_graph_ms=residual_ms,
               residual_repeats_ms=residual_reps, residual_round_ms=residual_round, temporal_round_ms=temporal_round,
               temporal_over_residual_round=temporal_round / residual_round, temporal_over_provider=total_ms / provider_ms,
               parse_with_temporal_ms=parse_again_ms, frames_per_s=R / (parse_again_ms * 1e-3), eager_launch_us=eager,
               pool_share_of_round=eager["air_temporal_pool"] / eager_round, score_share_of_round=eager["air_prune_score"] / eager_round,
               pool_bytes_moved=pool_bytes, pool_gb_per_s=pool_bytes / (eager["air_temporal_pool"] * 1e-6) / 1e9)
    print(json.dumps(res))
    for k, v in res.items():
        print("%-32s %s" % (k, v))
    tp.release_graphs(); pp.release_graphs(); ps.release_graphs()
    return res


if __name__ == "__main__":
    main()
