"""GPU tests of the MOTS measures (attend_infer_repeat_amd/track.py, csrc/track_kernels.hip): air_track_mots against
track.reference_mots -- all four outputs bit for bit --, the unchanged air_score_contingency in front of it, the argument checks, then
SequenceTracker.mots, TrackStitcher.mots, TrajectorySmoother.mots and the model's surface."""
import functools

import numpy as np
import pytest
import torch

from test_parse import _mnist_air
from test_track import dev_t, frames_for, make_tracker
from track_mots_cases import CRAFTED, mots_case, planted_case, table

from attend_infer_repeat_amd import track

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
POISON_F = -7.0e77
POISON_F32 = -3.0e33
TAIL = 64
OUT = track.MOTS_OUTPUTS
DTYPES = dict(seq_mots_i=torch.int32, seq_mots_f=torch.float64, mots_match=torch.int32, mots_iou=torch.float32)
FILL = dict(seq_mots_i=POISON, seq_mots_f=POISON_F, mots_match=POISON, mots_iou=POISON_F32)


def raw(a):
    """the bits of an array: float64 as int64, float32 as int32"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8).clone() if t.is_floating_point() else t.clone()


def shapes_of(S, R, G):
    return dict(seq_mots_i=(S, 8), seq_mots_f=(S,), mots_match=(R, G), mots_iou=(R, G))


def run_mots(case, maps=False, **kw):
    """air_track_mots alone on the case's table (maps=True: the unchanged air_score_contingency launch on the case's maps in front
    of it); every output and a tail behind it start as a sentinel fill"""
    from attend_infer_repeat_amd import hip as Hh
    T, G, S, F = case["T"], case["G"], case["S"], case["F"]
    R = S * F
    shapes = shapes_of(S, R, G)
    bufs = {k: torch.full((int(np.prod(v)) + TAIL,), FILL[k], dtype=DTYPES[k], device="cuda") for k, v in shapes.items()}
    L, p = Hh.lib(), Hh._p
    if maps:
        owner, gt = dev_t(case["owner"]), dev_t(case["gt"])
        cont = torch.full((R, T + 1, G + 1), POISON, dtype=torch.int32, device="cuda")
        Hi, Wi = case["owner"].shape[1:]
        assert L.air_score_contingency(p(owner), p(gt), T, G, R, Hi, Wi, p(cont), Hh._stream()) == 0
    else:
        cont = dev_t(table(case))
    d = dict(n=dev_t(case["n"].astype(np.int32)), ids=dev_t(case["ids"].astype(np.int32)))
    a = dict(cont=p(cont), n=p(d["n"]), ids=p(d["ids"]), T=T, G=G, S=S, F=F, R=R)
    a.update({k: p(bufs[k]) for k in shapes})
    a.update(kw)
    st = L.air_track_mots(a["cont"], a["n"], a["ids"], a["T"], a["G"], a["S"], a["F"], a["R"], a["seq_mots_i"], a["seq_mots_f"],
                          a["mots_match"], a["mots_iou"], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        got[k] = bufs[k][:n].view(shape).cpu().numpy()
        clean = clean and bool((bufs[k][n:] == FILL[k]).all())
    got["cont"] = cont.cpu().numpy()
    return st, got, clean


def reference(case):
    return track.reference_mots(table(case), case["n"], case["ids"], case["F"])


def check(got, want, where=""):
    for k in OUT:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (where, k)
        assert np.array_equal(raw(got[k]), raw(want[k])), (where, k, got[k], want[k])


@functools.lru_cache(maxsize=None)
def seeded(T, G, S, F):
    case = planted_case(T, G, S, F, seed=2 + T + G + S + F)
    return case, reference(case)


# ---- 1. air_track_mots ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,G,S,F", [(1, 1, 1, 1), (2, 2, 3, 4), (5, 3, 2, 8), (32, 8, 2, 3), (3, 8, 65, 2)])
def test_mots_is_the_reference(gpu_device, T, G, S, F):
    case, want = seeded(T, G, S, F)
    st, got, clean = run_mots(case)
    assert st == 0 and clean
    check(got, want)                                               # (every element written: no sentinel equals a reference value)
    total = dict(zip(track.MOTS_COUNTS, want["seq_mots_i"].astype(np.int64).sum(0).tolist()))
    print("T %d G %d S %d F %d: %r soft %.6f" % (T, G, S, F, total, want["seq_mots_f"].sum()))
    if (T, G, S, F) == (1, 1, 1, 1):
        assert total["tp"] == 1
    else:
        assert total["tp"] > 0 and total["fn"] > 0 and total["fp"] > 0 and total["ids"] > 0


def test_mots_on_the_big_table(gpu_device):
    case = CRAFTED["BIG"]
    st, got, clean = run_mots(case)
    assert st == 0 and clean
    check(got, reference(case), "BIG")
    assert got["mots_match"].tolist() == [[0]] and got["seq_mots_f"][0] == 1.6e9 / 2.7e9 and got["seq_mots_i"][0, :5].tolist() == [1, 1, 0, 0, 0]


def test_contingency_then_mots_on_seeded_maps(gpu_device):
    """the unchanged air_score_contingency in front: 7 x 13 = 91 pixels, so the rows of the maps are not 16-byte aligned"""
    for seed, (T, G, S, F) in enumerate([(3, 3, 3, 4), (5, 2, 2, 5), (2, 8, 4, 3)]):
        case = mots_case(T, G, S, F, seed=40 + seed, shape=(7, 13))
        cont = track.mots_contingency(case["owner"], case["gt"], T, G)
        want = track.reference_mots(cont, case["n"], case["ids"], F)
        st, got, clean = run_mots(case, maps=True)
        assert st == 0 and clean
        assert np.array_equal(got["cont"], cont), seed
        check(got, want, seed)
    assert want["seq_mots_i"][:, 1].sum() > 0


def test_mots_on_the_crafted_cases(gpu_device):
    for name, case in CRAFTED.items():
        st, got, clean = run_mots(case, maps="owner" in case)
        assert st == 0 and clean, name
        check(got, reference(case), name)
        have = dict(zip(track.MOTS_COUNTS, got["seq_mots_i"][0].tolist()), soft=float(got["seq_mots_f"][0]))
        assert have == case["want"], (name, have)
    got = run_mots(CRAFTED["EXACT_HALF"])[1]
    assert got["mots_match"].tolist() == [[-1]] and got["mots_iou"].tolist() == [[0.0]]
    got = run_mots(CRAFTED["FIVE_EIGHTHS"])[1]
    assert got["mots_match"].tolist() == [[0]] and got["mots_iou"].tolist() == [[0.625]] and got["seq_mots_f"].tolist() == [0.625]


def test_mots_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = planted_case(3, 2, 2, 4, seed=1)
    odd = torch.zeros(1024, dtype=torch.int32, device="cuda")
    odd8 = torch.zeros(1024, dtype=torch.int8, device="cuda")
    for kw, code in ((dict(cont=None), -1), (dict(n=None), -1), (dict(ids=None), -1), (dict(seq_mots_i=None), -1),
                     (dict(seq_mots_f=None), -1), (dict(mots_match=None), -1), (dict(mots_iou=None), -1),
                     (dict(T=0), -2), (dict(T=33), -2), (dict(G=0), -2), (dict(G=9), -2), (dict(S=0), -2), (dict(F=0), -2), (dict(R=9), -2),
                     (dict(S=-2, F=-4), -2),
                     (dict(T=32, G=8, S=4000, F=2000, R=8000000), -2),      # R (T+1) (G+1) beyond INT_MAX
                     (dict(seq_mots_f=Hh._p(odd[1:])), -3), (dict(cont=Hh._p(odd8[1:])), -3), (dict(n=Hh._p(odd8[2:])), -3),
                     (dict(ids=Hh._p(odd8[3:])), -3), (dict(seq_mots_i=Hh._p(odd8[1:])), -3), (dict(mots_match=Hh._p(odd8[2:])), -3),
                     (dict(mots_iou=Hh._p(odd8[1:])), -3),
                     (dict(cont=None, T=0), -1), (dict(T=0, seq_mots_f=Hh._p(odd[1:])), -2)):       # the family's order
        st, got, clean = run_mots(case, **kw)
        assert st == code, kw
        assert clean and all((got[k] == FILL[k]).all() for k in OUT), kw


# ---- 2. SequenceTracker.mots ------------------------------------------------------------------------------------------------------------
def plant(owner, counts, ids, case):
    """the case's owner maps, counts and ids into a stage's buffers (what a MOTS table reads)"""
    owner.copy_(torch.from_numpy(case["owner"]).reshape(owner.shape))
    counts.copy_(torch.from_numpy(case["n"]))
    ids.copy_(torch.from_numpy(case["ids"]))
    torch.cuda.synchronize()


def test_tracker_mots_eager_graph_totals_and_the_other_metrics_are_untouched(gpu_device):
    S, F, G = 3, 5, 2
    ocfg, eager, pe = make_tracker("rect_t5", S, F, birth_score=0.0)
    _, graph, pg = make_tracker("rect_t5", S, F, capture=True, birth_score=0.0)
    T, R, img = ocfg.max_steps, S * F, tuple(ocfg.img_size)
    frames = frames_for(ocfg, S, F, 31).cuda()
    eager.track(frames), graph.track(frames)
    eager.synchronize(); graph.synchronize()
    case = mots_case(T, G, S, F, seed=5, shape=img)
    for tk, pr in ((eager, pe), (graph, pg)):                      # planted rows: what the table reads is the case's
        plant(pr.owner, pr.num_objects, tk.track_id, case)
    gt_boxes = torch.rand(S, F, G, 4) * 10 + 1
    # score(), score(identity=True) and hota() before ...
    before = {i: {k: bits(v) for k, v in graph.score(gt_boxes, accumulate=False, identity=i).items()} for i in (False, True)}
    hota_before = {k: bits(v) for k, v in graph.hota(gt_boxes, accumulate=False).items()}
    keys, entries, hota_entries = list(graph._score), list(graph._score.values()), list(graph.scores.hota_entries.values())
    want = track.reference_mots(track.mots_contingency(case["owner"], case["gt"], T, G), case["n"], case["ids"], F)
    gi = torch.from_numpy(case["gt"])
    a = eager.mots(gi, G, accumulate=False)
    b = graph.mots(gi.reshape(S, F, *img).cuda(), G, accumulate=False)
    eager.synchronize(); graph.synchronize()
    assert set(b) == set(OUT) | {"cont", "totals_mots_i", "totals_mots_f"}
    entry = graph.scores.mots_entries[(G,)]
    assert [e[2] for e in entry["plan"]] == ["air_score_contingency", "air_track_mots"] and entry["graph"] is not None
    assert eager.scores.mots_entries[(G,)]["graph"] is None and entry["gt_instances"].dtype == torch.int8
    for k in OUT + ("cont",):                                      # eager = captured replay, bit for bit, = the reference
        assert torch.equal(bits(a[k]), bits(b[k])), k
    check({k: b[k].cpu().numpy() for k in OUT}, want)
    assert want["seq_mots_i"][:, 1].sum() > 0 and want["seq_mots_i"][:, 3].sum() > 0
    assert b["totals_mots_i"].dtype == torch.int64 and b["totals_mots_f"].dtype == torch.float64
    assert b["totals_mots_i"].tolist() == want["seq_mots_i"].astype(np.int64).sum(0).tolist()
    # the total of S per-sequence sums is added on the device in an order of its own: S + 1 roundings at most on either side
    soft, close = float(want["seq_mots_f"].sum()), lambda x, y: abs(x - y) <= (S + 1) * np.finfo(np.float64).eps * abs(y)
    assert close(float(b["totals_mots_f"]), soft)
    once = graph.mots_summary()
    assert once == track.mots_summary(want["seq_mots_i"].astype(np.int64).sum(0), float(b["totals_mots_f"]))
    print("tracker motsa %.4f smotsa %.4f motsp %.4f" % (once["motsa"], once["smotsa"], once["motsp"]))
    # ... and after: the same bits, the same caches
    for i in (False, True):
        again = graph.score(gt_boxes, accumulate=False, identity=i)
        assert set(again) == set(before[i]) and all(torch.equal(bits(again[k]), before[i][k]) for k in again), i
    again = graph.hota(gt_boxes, accumulate=False)
    assert all(torch.equal(bits(again[k]), hota_before[k]) for k in again)
    assert list(graph._score) == keys and all(x is y for x, y in zip(graph._score.values(), entries))
    assert all(x is y for x, y in zip(graph.scores.hota_entries.values(), hota_entries)) and len(graph.scores.mots_entries) == 1
    # a second batch accumulates; accumulate=False restarts; reset() zeroes
    case2 = mots_case(T, G, S, F, seed=6, shape=img)
    plant(pg.owner, pg.num_objects, graph.track_id, case2)
    want2 = track.reference_mots(track.mots_contingency(case2["owner"], case2["gt"], T, G), case2["n"], case2["ids"], F)
    c = graph.mots(torch.from_numpy(case2["gt"]), G, accumulate=True)
    graph.synchronize()
    check({k: c[k].cpu().numpy() for k in OUT}, want2)
    assert c["totals_mots_i"].tolist() == (want["seq_mots_i"].astype(np.int64).sum(0) + want2["seq_mots_i"].sum(0)).tolist()
    assert close(float(c["totals_mots_f"]), soft + float(want2["seq_mots_f"].sum()))
    c = graph.mots(torch.from_numpy(case2["gt"]), G, accumulate=False)
    graph.synchronize()
    assert c["totals_mots_i"].tolist() == want2["seq_mots_i"].astype(np.int64).sum(0).tolist()
    assert close(float(c["totals_mots_f"]), float(want2["seq_mots_f"].sum()))
    hota_total = graph.scores.totals_hota_i.clone()
    graph.reset()
    assert not graph.scores.totals_mots_i.any() and not graph.scores.totals_mots_f.any() and np.isnan(graph.mots_summary()["motsa"])
    assert hota_total.any() and not graph.scores.totals_hota_i.any()
    for g in (1, 3, 2):                                            # the cap of two entries
        graph.mots(gi, g)
    assert list(graph.scores.mots_entries) == [(3,), (2,)] and list(graph._score) == keys
    with pytest.raises(ValueError, match="gt_instances"):
        graph.mots(torch.zeros(S * F + 1, *img, dtype=torch.int8), G)
    with pytest.raises(ValueError, match="ground-truth slots"):
        graph.mots(gi, 9)
    graph.release_graphs()
    assert all(e["graph"] is None for e in graph.scores.mots_entries.values())
    graph.capture()
    assert all(e["graph"] is not None for e in graph.scores.mots_entries.values())
    graph.release_graphs()
    assert not hasattr(track.StreamTracker, "mots")


# ---- 3. the stitcher and the smoother -----------------------------------------------------------------------------------------------------
def test_stitcher_and_smoother_mots_on_their_own_tables(gpu_device):
    from attend_infer_repeat_amd.track import TrackStitcher
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    S, F, G = 2, 4, 3
    ocfg, tk, pr = make_tracker("tiny", S, F, capture=True, birth_score=0.0)
    T, img = ocfg.max_steps, tuple(ocfg.img_size)
    frames = frames_for(ocfg, S, F, 7).cuda()
    st, sm = TrackStitcher(tk), TrajectorySmoother(tk)
    st.capture(); sm.capture()
    st.stitch(frames)
    sm.run()
    st.synchronize(); sm.synchronize()
    # the stitcher: the provider's owner map and counts with ITS ids (the tracker's ids hold another case's)
    case, other = mots_case(T, G, S, F, seed=21, shape=img), mots_case(T, G, S, F, seed=22, shape=img)
    plant(pr.owner, pr.num_objects, st.stitch_id, case)
    tk.track_id.copy_(torch.from_numpy(other["ids"]))
    gi = torch.from_numpy(case["gt"])
    got = st.mots(gi, G, accumulate=False)
    st.synchronize()
    cont = track.mots_contingency(case["owner"], case["gt"], T, G)
    want = track.reference_mots(cont, case["n"], case["ids"], F)
    check({k: got[k].cpu().numpy() for k in OUT}, want, "stitched")
    assert np.array_equal(got["cont"].cpu().numpy(), cont) and want["seq_mots_i"][:, 1].sum() > 0
    assert st.mots_summary() == track.mots_summary(want["seq_mots_i"].astype(np.int64).sum(0), float(st.scores.totals_mots_f))
    assert abs(float(st.scores.totals_mots_f) - float(want["seq_mots_f"].sum())) <= 1e-12
    assert st.scores.mots_entries[(G,)]["graph"] is not None and not tk.scores.mots_entries and not tk.scores.totals_mots_i.any()
    raw_ids = tk.mots(gi, G, accumulate=False)
    tk.synchronize()
    check({k: raw_ids[k].cpu().numpy() for k in OUT}, track.reference_mots(cont, case["n"], other["ids"], F), "tracker")
    # the smoother: the completed table's owner map, counts and ids, T := C
    C = sm.C
    done = mots_case(C, G, S, F, seed=23, shape=img)
    plant(sm.sm["owner"], sm.sm["count"], sm.sm["id"], done)
    got = sm.mots(torch.from_numpy(done["gt"]).reshape(S, F, *img), G, accumulate=False)
    sm.synchronize()
    want = track.reference_mots(track.mots_contingency(done["owner"], done["gt"], C, G), done["n"], done["ids"], F)
    check({k: got[k].cpu().numpy() for k in OUT}, want, "completed")
    assert tuple(got["cont"].shape) == (S * F, C + 1, G + 1) and want["seq_mots_i"][:, 1].sum() > 0
    assert sm.scores.mots_entries[("completed", G)]["graph"] is not None and sm.scores is not tk.scores
    assert sm.mots_summary() == track.mots_summary(want["seq_mots_i"].astype(np.int64).sum(0), float(sm.scores.totals_mots_f))
    assert abs(float(sm.scores.totals_mots_f) - float(want["seq_mots_f"].sum())) <= 1e-12
    sm.reset()
    assert np.isnan(sm.mots_summary()["motsa"]) and not np.isnan(st.mots_summary()["motsa"])
    st.release_graphs(); sm.release_graphs(); tk.release_graphs()


# ---- 4. the model, the logger, the script ---------------------------------------------------------------------------------------------------
def same_figures(a, b):
    """two mots_summary dicts with equal values, nan equal to nan"""
    return set(a) == set(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def host_mots(owner, count, ids, gi, F, G):
    owner = owner.cpu().numpy()
    T = ids.shape[0]
    cont = track.mots_contingency(owner, np.asarray(gi).reshape(owner.shape), T, G)
    return track.reference_mots(cont, count.cpu().numpy(), ids.cpu().numpy(), F)


def test_score_track_mots_on_moving_mnist(gpu_device):
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    S, F = 4, 4
    air, ts, x, y = _mnist_air(8)
    ts()
    raw_data = procedural_moving_mnist(S, F, canvas_size=(50, 50), n_objects=(1, 2), seed=3, n_templates=64, return_annotations=True)
    frames = torch.from_numpy(raw_data["imgs"].astype("float32") / 255.0).cuda()
    gb, gi = torch.from_numpy(raw_data["boxes"]), torch.from_numpy(raw_data["instances"])
    G = int(gb.shape[-2])
    kw = dict(accumulate=False, birth_score=0.0)
    with pytest.raises(ValueError, match="mots=True scores the tracks as masks"):
        air.score_track(frames, gb, mots=True, **kw)
    plain, tk = air.score_track(frames, gb, gt_instances=gi, **kw)
    assert "mots" not in plain and not tk.scores.mots_entries      # the default: today's call
    scores, tk2 = air.score_track(frames, gb, gt_instances=gi, mots=True, **kw)
    assert tk2 is tk and set(scores) == set(plain) | {"mots"}
    tk.synchronize()
    out = air.tracked
    want = host_mots(out["owner"], out["num_objects"], out["track_id"], gi, F, G)
    check({k: scores["mots"][k].cpu().numpy() for k in OUT}, want, "raw")
    fig = tk.mots_summary()
    assert same_figures(fig, track.mots_summary(want["seq_mots_i"].astype(np.int64).sum(0), float(tk.scores.totals_mots_f)))
    assert abs(fig["soft"] - float(want["seq_mots_f"].sum())) <= 1e-12      # (S = 4 sums below 8 each, added in the device's order)
    assert fig["gt"] == int((raw_data["instances"].reshape(S * F, -1)[:, :, None] == np.arange(G)).any(1).sum())
    print("moving mnist, untrained: motsa %.4f smotsa %.4f tp %d fp %d gt %d" % (fig["motsa"], fig["smotsa"], fig["tp"],
                                                                                 fig["false_positives"], fig["gt"]))
    # the same frames against instance maps cut from the parse's own owner map: every step below G with a track and a pixel matches
    own = out["owner"].cpu().numpy()
    cut = torch.from_numpy(np.where(own < G, own, -1).astype(np.int8)).reshape(S, F, 50, 50)
    scores, _ = air.score_track(frames, gb, gt_instances=cut, mots=True, **kw)
    tk.synchronize()
    assert np.array_equal(air.tracked["owner"].cpu().numpy(), own)
    want = host_mots(out["owner"], out["num_objects"], out["track_id"], cut, F, G)
    check({k: scores["mots"][k].cpu().numpy() for k in OUT}, want, "cut")
    fig = tk.mots_summary()
    print("the parse's own masks: motsa %.4f smotsa %.4f tp %d fp %d fn %d gt %d" % (fig["motsa"], fig["smotsa"], fig["tp"],
                                                                                   fig["false_positives"], fig["misses"], fig["gt"]))
    assert fig["tp"] == int(want["seq_mots_i"][:, 1].sum()) and (fig["tp"] == 0 or fig["motsp"] == 1.0)
    # with smooth=: the completed table beside the raw one
    scores, tk3 = air.score_track(frames, gb, gt_instances=gi, mots=True, smooth=True, **kw)
    sm = air.track_smoother
    sm.synchronize()
    out = air.tracked
    assert set(scores["completed"]) >= {"mots", "seq_counts"}
    check({k: scores["mots"][k].cpu().numpy() for k in OUT}, host_mots(out["owner"], out["num_objects"], out["track_id"], gi, F, G), "raw")
    check({k: scores["completed"]["mots"][k].cpu().numpy() for k in OUT},
          host_mots(out["sm_owner"], out["sm_count"], out["sm_id"], gi, F, G), "completed")
    # with stitch=: the stitched ids are scored
    scores, st = air.score_track(frames, gb, gt_instances=gi, mots=True, stitch=True, **kw)
    st.synchronize()
    out = air.tracked
    assert isinstance(st, track.TrackStitcher)
    check({k: scores["mots"][k].cpu().numpy() for k in OUT}, host_mots(out["owner"], out["num_objects"], out["stitch_id"], gi, F, G),
          "stitched")
    assert st.scores.totals_mots_i.any() and not st.tracker.scores.mots_entries      # the stitcher's totals, not the tracker's


def test_track_score_logger_and_script_option(gpu_device, tmp_path, capsys):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "2", "--log-every", "2", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5",
                            "--track-mots", "--track-smooth"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert len(rec) == 2 and printed.count(" motsa = ") == 2 and printed.count(" smotsa = ") == 2 and printed.count(" motsp = ") == 2
    assert printed.count("smooth_smotsa = ") == 2
    for l in rec:
        for k in ("motsa", "smotsa", "smooth_smotsa"):
            assert k in l and (l[k] <= 1.0 or np.isnan(l[k])), (k, l[k])
        assert "motsp" in l and (0.5 < l["motsp"] <= 1.0 or np.isnan(l["motsp"])) and "hota" not in l
    for argv in (["--track-mots"], ["--track-eval", "4", "--track-stream", "2", "--track-mots"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(argv)
    err = capsys.readouterr().err
    assert "--track-mots goes with --track-eval" in err and "MOTS is out of scope on a stream" in err
