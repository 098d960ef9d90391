"""GPU tests of the HOTA metric (attend_infer_repeat_amd/track.py, csrc/track_kernels.hip): air_track_hota against
track.reference_hota -- the integer outputs exactly, the float64 outputs by bits --, then SequenceTracker.hota, TrajectorySmoother.hota
and the model's surface."""
import functools

import numpy as np
import pytest
import torch

from test_parse import _mnist_air
from test_track import dev_t, frames_for, host_rows, make_tracker
from test_track_host import moving_gt
from track_hota_cases import CRAFTED, hota_case

from attend_infer_repeat_amd import track

pytestmark = pytest.mark.gpu

NA = 19
POISON = 0x5A5A5A5A
POISON_F = -7.0e77
TAIL = 64
OUT = ("hota_potential", "hota_id_count", "hota_gt_count", "hota_matches", "seq_hota_i", "seq_hota_f")
FLOATS = ("hota_potential", "seq_hota_f")
bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)


def shapes_of(S, G, n_ids):
    return dict(hota_potential=(S, G, n_ids), hota_id_count=(S, n_ids), hota_gt_count=(S, G), hota_matches=(S, NA, G, n_ids),
                seq_hota_i=(S, NA, 3), seq_hota_f=(S, NA, 4))


def run_hota(case, n_ids=None, **kw):
    """air_track_hota alone (current stream); every output and a tail behind it start as a sentinel fill"""
    from attend_infer_repeat_amd import hip as Hh
    T, S, F, G = case["T"], case["S"], case["F"], case["G"]
    R = S * F
    n_ids = case.get("n_ids", F * T) if n_ids is None else n_ids
    shapes = shapes_of(S, G, n_ids)
    bufs = {k: torch.full((int(np.prod(v)) + TAIL,), POISON_F if k in FLOATS else POISON,
                          dtype=torch.float64 if k in FLOATS else torch.int32, device="cuda") for k, v in shapes.items()}
    d = dict(boxes=dev_t(case["boxes"]), n=dev_t(case["n"].astype(np.int32)), ids=dev_t(case["ids"].astype(np.int32)), gt=dev_t(case["gt"]))
    p = Hh._p
    a = dict(boxes=p(d["boxes"]), n=p(d["n"]), ids=p(d["ids"]), gt=p(d["gt"]), T=T, G=G, S=S, F=F, R=R, n_ids=n_ids)
    a.update({k: p(bufs[k]) for k in shapes})
    a.update(kw)
    st = Hh.lib().air_track_hota(a["boxes"], a["n"], a["ids"], a["gt"], a["T"], a["G"], a["S"], a["F"], a["R"], a["n_ids"],
                                 a["hota_potential"], a["hota_id_count"], a["hota_gt_count"], a["hota_matches"], a["seq_hota_i"],
                                 a["seq_hota_f"], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        got[k] = bufs[k][:n].view(shape).cpu().numpy()
        clean = clean and bool((bufs[k][n:] == (POISON_F if k in FLOATS else POISON)).all())
    return st, got, clean


def reference(case, n_ids=None):
    return track.reference_hota(case["boxes"], case["n"], case["ids"], case["gt"], case["F"], case.get("n_ids") if n_ids is None else n_ids)


def check(got, want, where=""):
    for k in OUT:
        assert got[k].shape == want[k].shape, (where, k)
        if k in FLOATS:
            assert np.array_equal(bits64(got[k]), bits64(want[k])), (where, k, np.abs(got[k] - want[k]).max())
        else:
            assert np.array_equal(got[k], want[k]), (where, k)


@functools.lru_cache(maxsize=None)
def seeded(T, G, S, F):
    case = hota_case(T, S, F, G, seed=T + G + S + F, followers=4 if T == 32 else 1)
    return case, reference(case)


# ---- 1. air_track_hota ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,G,S,F", [(3, 2, 3, 5), (1, 1, 2, 1), (6, 8, 2, 17), (32, 8, 2, 3), (6, 3, 2, 48)])
def test_hota_is_the_reference(gpu_device, T, G, S, F):
    case, want = seeded(T, G, S, F)
    st, got, clean = run_hota(case)
    assert st == 0 and clean
    check(got, want)                                               # (every element written: no sentinel equals a reference value)
    fig = track.hota_summary(want["seq_hota_i"].sum(0), want["seq_hota_f"].sum(0))
    print("T %d G %d S %d F %d: tp %s hota %.4f deta %.4f assa %.4f; hypotheses per frame up to %d" % (
        T, G, S, F, want["seq_hota_i"][:, 0, 0].tolist(), fig["hota"], fig["deta"], fig["assa"], (case["ids"] >= 0).sum(0).max()))
    if (T, G, S, F) != (1, 1, 2, 1):
        assert want["seq_hota_i"][:, 0, 0].min() > 0 and want["hota_matches"].max() >= 1
    if T == 32:
        assert (case["ids"] >= 0).sum(0).max() >= 31               # every lane of the solver and of the pair loop
    if F == 48:
        assert want["hota_id_count"].shape[1] == 288 and want["hota_id_count"][:, 256:].any()       # ids behind the 256th take part


def test_hota_with_a_table_smaller_than_the_largest_id(gpu_device):
    case, _ = seeded(6, 8, 2, 17)
    assert case["ids"].max() >= 40
    for n_ids in (40, 1):
        want = reference(case, n_ids)
        st, got, clean = run_hota(case, n_ids)
        assert st == 0 and clean
        check(got, want, n_ids)
    assert want["seq_hota_i"][:, 0, 2].min() > 0                   # the hypotheses beyond the table are false positives


def test_hota_on_the_crafted_cases(gpu_device):
    for name, case in CRAFTED.items():
        st, got, clean = run_hota(case)
        assert st == 0 and clean, name
        check(got, reference(case), name)
    got = run_hota(CRAFTED["SPLIT"])[1]
    fig = track.hota_summary(got["seq_hota_i"][0], got["seq_hota_f"][0])
    assert fig["deta"] == 1.0 and fig["assa"] == 0.5
    got = run_hota(CRAFTED["EXACT_LEVELS"])[1]
    assert got["seq_hota_i"][0, :, 0].tolist() == [3] * 5 + [2] * 5 + [1] * 5 + [0] * 4
    got = run_hota(CRAFTED["PROFIT_TIE"])[1]
    assert got["hota_matches"][0, 0, 0].tolist()[:2] == [0, 2]     # the tie rule: the hypothesis inserted second keeps the slot


def test_hota_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = hota_case(3, 2, 4, 2, seed=1)
    off = torch.zeros(2 * 8 * 4 + 1, device="cuda")
    odd = torch.zeros(1024, dtype=torch.int32, device="cuda")
    for kw, code in ((dict(boxes=None), -1), (dict(n=None), -1), (dict(ids=None), -1), (dict(gt=None), -1), (dict(hota_potential=None), -1),
                     (dict(hota_id_count=None), -1), (dict(hota_gt_count=None), -1), (dict(hota_matches=None), -1),
                     (dict(seq_hota_i=None), -1), (dict(seq_hota_f=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(G=0), -2),
                     (dict(G=9), -2), (dict(S=0), -2), (dict(F=0), -2), (dict(R=9), -2), (dict(n_ids=0), -2), (dict(n_ids=32768), -2),
                     (dict(S=2000, F=4, R=8000, n_ids=32767), -2),     # S 19 G n_ids beyond INT_MAX
                     (dict(gt=Hh._p(off[1:])), -3), (dict(boxes=Hh._p(off[1:])), -3), (dict(seq_hota_f=Hh._p(odd[1:])), -3),
                     (dict(hota_potential=Hh._p(odd[1:])), -3)):
        st, got, clean = run_hota(case, **kw)
        assert st == code, kw
        assert clean and all((got[k] == (POISON_F if k in FLOATS else POISON)).all() for k in got), kw


# ---- 2. SequenceTracker.hota ------------------------------------------------------------------------------------------------------------
def test_tracker_hota_eager_graph_totals_and_score_is_untouched(gpu_device):
    S, F, G = 3, 5, 2
    ocfg, eager, _ = make_tracker("rect_t5", S, F, birth_score=0.0, matching="optimal")
    _, graph, _ = make_tracker("rect_t5", S, F, capture=True, birth_score=0.0, matching="optimal")
    T, R = ocfg.max_steps, S * F
    frames = frames_for(ocfg, S, F, 31).cuda()
    out_e, out = eager.track(frames), graph.track(frames)
    eager.synchronize(); graph.synchronize()
    rows, ids = host_rows(out, T, R), out["track_id"].cpu().numpy()
    gt = moving_gt(dict(boxes=rows["boxes"], n=rows["n"], T=T, S=S, F=F), np.random.default_rng(1), G).reshape(S, F, G, 4)
    gt_t = torch.from_numpy(gt)
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8).clone() if t.is_floating_point() else t.clone()
    # score() and score(identity=True) before ...
    before = {i: {k: raw(v) for k, v in graph.score(gt_t, accumulate=False, identity=i).items()} for i in (False, True)}
    keys, entries = list(graph._score), list(graph._score.values())
    want = track.reference_hota(rows["boxes"], rows["n"], ids, gt, F)
    a, b = eager.hota(gt_t, accumulate=False), graph.hota(gt_t.cuda(), accumulate=False)
    eager.synchronize(); graph.synchronize()
    assert set(b) == set(OUT) | {"totals_hota_i", "totals_hota_f"}
    entry = graph.scores.hota_entries[(G,)]
    assert [e[2] for e in entry["plan"]] == ["air_track_hota"] and entry["graph"] is not None
    assert eager.scores.hota_entries[(G,)]["graph"] is None
    for k in OUT:                                                  # eager = captured replay, bit for bit, = the reference
        assert torch.equal(raw(a[k]), raw(b[k])), k
    check({k: b[k].cpu().numpy() for k in OUT}, want)
    assert tuple(b["hota_matches"].shape) == (S, NA, G, F * T) and want["seq_hota_i"][:, 0, 0].sum() > 0
    assert b["totals_hota_i"].dtype == torch.int64 and b["totals_hota_f"].dtype == torch.float64
    assert b["totals_hota_i"].tolist() == want["seq_hota_i"].sum(0).tolist()
    sums = torch.from_numpy(want["seq_hota_f"]).sum(0)
    assert torch.equal(b["totals_hota_f"].cpu(), sums)
    once = graph.hota_summary()
    ref_fig = track.hota_summary(want["seq_hota_i"].sum(0), sums.numpy())
    assert once == ref_fig and 0.0 < once["hota"] <= 1.0 and len(once["per_alpha"]["hota"]) == NA
    print("tracker hota %.4f deta %.4f assa %.4f loca %.4f" % (once["hota"], once["deta"], once["assa"], once["loca"]))
    # ... and after: the same bits, the same cache
    for i in (False, True):
        again = graph.score(gt_t, accumulate=False, identity=i)
        assert set(again) == set(before[i]) and all(torch.equal(raw(again[k]), before[i][k]) for k in again), i
    assert list(graph._score) == keys and all(x is y for x, y in zip(graph._score.values(), entries))
    assert all("hota" not in str(k) for k in graph._score) and len(graph.scores.hota_entries) == 1
    # a second batch accumulates; reset() zeroes
    frames2 = frames_for(ocfg, S, F, 32).cuda()
    out2 = graph.track(frames2)
    graph.synchronize()
    rows2 = host_rows(out2, T, R)
    want2 = track.reference_hota(rows2["boxes"], rows2["n"], out2["track_id"].cpu().numpy(), gt, F)
    c = graph.hota(gt_t, accumulate=True)
    graph.synchronize()
    check({k: c[k].cpu().numpy() for k in OUT}, want2)
    assert c["totals_hota_i"].tolist() == (want["seq_hota_i"].sum(0) + want2["seq_hota_i"].sum(0)).tolist()
    assert torch.equal(c["totals_hota_f"].cpu(), sums + torch.from_numpy(want2["seq_hota_f"]).sum(0))
    mota_before = graph.summary()["gt"]
    graph.reset()
    assert not graph.scores.totals_hota_i.any() and not graph.scores.totals_hota_f.any() and np.isnan(graph.hota_summary()["hota"])
    assert graph.summary()["gt"] == 0 and mota_before > 0
    for g in (1, 3, 2):                                            # the cap of two entries
        graph.hota(torch.zeros(S, F, g, 4))
    assert list(graph.scores.hota_entries) == [(3,), (2,)] and list(graph._score) == keys
    with pytest.raises(ValueError, match="gt_boxes"):
        graph.hota(torch.zeros(S * F + 1, G, 4))
    with pytest.raises(ValueError, match="ground-truth slots"):
        graph.hota(torch.zeros(S, F, 9, 4))
    graph.release_graphs()
    assert all(e["graph"] is None for e in graph.scores.hota_entries.values())
    assert not hasattr(track.StreamTracker, "hota")


# ---- 3. the smoother and the model ------------------------------------------------------------------------------------------------------
def test_score_track_hota_on_planted_rows_raw_and_completed(gpu_device):
    """AIRonMNIST.score_track(hota=True, smooth=) with the planted linear sequences in the provider's buffers (every track has ONE
    interior sighting removed, max_age = 1): the tracker's HOTA is the reference on the tracker's own output, the smoother's the
    reference on the completed table, and the completed table -- the gap filled -- has the higher DetA"""
    from test_trajectory import plant
    from trajectory_cases import PLANTED, planted_sequences
    S, F, K, Hz = PLANTED["S"], PLANTED["F"], PLANTED["K"], PLANTED["HZ"]
    air, ts, x, y = _mnist_air(8)
    ts()
    case, gt, gt_future, gaps = planted_sequences(A=50, G=400)
    frames = torch.zeros(S, F, 50, 50).cuda()
    spec = dict(horizon=Hz)
    sm = air.trajectory_smoother(S, F, spec)
    inner = sm.provider.parse

    def planted_parse(*args, **kwargs):
        base = inner(*args, **kwargs)
        plant(sm.provider, case)
        return base

    sm.provider.parse = planted_parse
    plain, tk = air.score_track(frames, gt, accumulate=False, smooth=spec)
    assert "hota" not in plain and "hota" not in plain["completed"] and not tk.scores.hota_entries      # the default: today's call
    scores, tk2 = air.score_track(frames, gt, accumulate=False, smooth=spec, hota=True)
    assert tk2 is tk and tk is sm.tracker and set(scores) == set(plain) | {"hota"}
    assert set(scores["completed"]) == set(plain["completed"]) | {"hota"}
    tk.synchronize()
    out = air.tracked
    T = tk.T
    want = track.reference_hota(out["boxes"].cpu().numpy(), out["num_objects"].cpu().numpy(), out["track_id"].cpu().numpy(), gt, F)
    check({k: scores["hota"][k].cpu().numpy() for k in OUT}, want, "raw")
    done = track.reference_hota(out["sm_boxes"].cpu().numpy(), out["sm_count"].cpu().numpy(), out["sm_id"].cpu().numpy(), gt, F, F * T)
    check({k: scores["completed"]["hota"][k].cpu().numpy() for k in OUT}, done, "completed")
    raw_fig, done_fig = tk.hota_summary(), sm.hota_summary()
    print("planted: raw hota %.4f deta %.4f assa %.4f; completed hota %.4f deta %.4f assa %.4f" % (
        raw_fig["hota"], raw_fig["deta"], raw_fig["assa"], done_fig["hota"], done_fig["deta"], done_fig["assa"]))
    assert raw_fig == track.hota_summary(want["seq_hota_i"].sum(0), want["seq_hota_f"].sum(0))
    assert want["seq_hota_i"][:, 0, 1].sum() == gaps and done["seq_hota_i"][:, 0, 1].sum() == 0       # one miss per gap; none once filled
    assert done_fig["deta"] > raw_fig["deta"] and raw_fig["gt_dets"] == done_fig["gt_dets"] == S * F * K
    assert sm.scores.hota_entries[("completed", K)]["graph"] is not None and sm.scores is not tk.scores
    ahead = sm.hota_forecast(torch.from_numpy(gt_future))
    sm.synchronize()
    fwant = track.reference_hota(out["fc_boxes"].cpu().numpy(), out["fc_count"].cpu().numpy(), out["fc_id"].cpu().numpy(), gt_future,
                                 Hz, F * T)
    check({k: ahead[k].cpu().numpy() for k in OUT}, fwant, "forecast")
    assert "totals_hota_i" not in ahead and fwant["seq_hota_i"][:, 0, 0].sum() == S * Hz * K
    assert list(sm.scores.hota_entries) == [("completed", K), ("forecast", K)]
    sm.reset()
    assert np.isnan(sm.hota_summary()["hota"]) and tk.hota_summary() == raw_fig


def test_track_score_logger_and_script_option(gpu_device, tmp_path, capsys):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "2", "--log-every", "2", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5",
                            "--track-hota", "--track-smooth"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert len(rec) == 2 and printed.count(" hota = ") == 2 and printed.count("smooth_hota = ") == 2
    for l in rec:
        for k in ("hota", "deta", "assa", "loca", "smooth_hota"):
            assert k in l and (0.0 <= l[k] <= 1.0 or np.isnan(l[k])), (k, l[k])
        assert "idf1" not in l
    for argv in (["--track-hota"], ["--track-eval", "4", "--track-stream", "2", "--track-hota"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(argv)
    err = capsys.readouterr().err
    assert "--track-hota goes with --track-eval" in err and "HOTA is out of scope on a stream" in err
