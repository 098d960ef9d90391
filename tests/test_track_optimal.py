"""GPU tests of the optimal association and the IDF1 metric (attend_infer_repeat_amd/track.py, csrc/track_kernels.hip):
air_track_associate_optimal against track.reference_associate(matching="optimal") on every output (affinity by bits),
air_track_idf against track.reference_identity exactly, then SequenceTracker(matching="optimal"), score(identity=True) and the
model's surface."""
import numpy as np
import pytest
import torch

from test_parse import _mnist_air, _train_state
from test_track import (DTYPES, MARGIN, bits, check_associate, dev_t, frames_for, host_rows, make_tracker, owner_reference, run_associate,
                        sentinel)
from test_track_host import OUTPUTS, crafted_rows, moving_gt
from track_optimal_cases import CHAIN, TIE_ONE_TRACK, TIE_TWO_TRACKS, WORKED, crafted_optimal, full_table_rows, identity_case, planted

from attend_infer_repeat_amd import track

pytestmark = pytest.mark.gpu


# ---- 1. air_track_associate_optimal -------------------------------------------------------------------------------------------------
def run_optimal(case, **kw):
    """air_track_associate_optimal alone (current stream); every output and a tail behind it start as a sentinel fill"""
    from attend_infer_repeat_amd import hip as Hh
    T, A, S, F = case["T"], case["A"], case["S"], case["F"]
    R = S * F
    shapes = dict(track_id=(T, R), obj_state=(T, R), affinity=(T, R), prev_frame=(T, R), prev_slot=(T, R), num_tracks=(S,),
                  track_first=(S, F * T), track_last=(S, F * T), track_length=(S, F * T), track_gaps=(S, F * T), state_counts=(S, 6))
    bufs = {k: sentinel(shapes[k], DTYPES[k]) for k in OUTPUTS}
    d = {k: dev_t(case[k]) for k in ("what", "boxes", "score")}
    d["n"] = dev_t(case["n"].astype(np.int32))
    p = Hh._p
    assoc = dict(track.DEFAULTS)
    assoc.update(case.get("kw", {}))
    a = dict(what=p(d["what"]), boxes=p(d["boxes"]), score=p(d["score"]), n=p(d["n"]), T=T, S=S, F=F, R=R, A=A, **assoc)
    a.update({k: p(bufs[k][0]) for k in OUTPUTS})
    a.update(kw)
    st = Hh.lib().air_track_associate_optimal(a["what"], a["boxes"], a["score"], a["n"], a["T"], a["S"], a["F"], a["R"], a["A"],
                                              float(a["iou_gate"]), float(a["appearance_weight"]), float(a["birth_score"]),
                                              int(a["max_age"]), *[a[k] for k in OUTPUTS], Hh._stream())
    torch.cuda.synchronize()
    got, tails = {}, {}
    for k in OUTPUTS:
        n = int(np.prod(shapes[k]))
        got[k], tails[k] = bufs[k][0][:n].view(shapes[k]).cpu().numpy(), bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, tails, {k: bufs[k][1] for k in OUTPUTS}


@pytest.mark.parametrize("T,A,S,F", [(3, 5, 3, 5), (1, 4, 2, 3), (6, 50, 2, 17), (3, 5, 4, 1)])
def test_optimal_associate_is_the_reference(gpu_device, T, A, S, F):
    kw = dict(iou_gate=0.2, appearance_weight=0.6, birth_score=0.4, max_age=2) if (T + A + S + F) % 2 else {}
    case, ref = crafted_optimal(T, A, S, F, seed=T + A + S + F, **kw)
    st, got, tails, _ = run_optimal(case)
    assert st == 0
    check_associate(got, ref, tails)
    print("states", ref["state_counts"].sum(0).tolist(), "tracks", ref["num_tracks"].tolist())
    assert (got["state_counts"].sum(1) == T * F).all()


@pytest.mark.parametrize("name,spread,kw", [("every pair admissible", 1.5, dict(iou_gate=0.0, appearance_weight=0.5)),
                                            ("sparse gating", 40.0, dict(iou_gate=0.3, appearance_weight=0.5))])
def test_optimal_associate_with_all_32_slots_live(gpu_device, name, spread, kw):
    case = full_table_rows(F=4, seed=3, spread=spread)
    case["kw"] = kw
    args = (case["what"], case["boxes"], case["score"], case["n"], 4)
    ref = track.reference_associate(*args, return_margins=True, matching="optimal", **kw)
    greedy = track.reference_associate(*args, **kw)
    assert ref["gate_margin"][0] >= MARGIN and ref["state_counts"][0, track.BORN] >= 32      # all 32 slots live from frame 0 on
    matched = int(ref["state_counts"][0, track.MATCHED])
    print(name, "matched", matched, "of 96; greedy matched", int(greedy["state_counts"][0, track.MATCHED]))
    assert matched == 96 if spread < 2 else matched > 0         # (every pair admissible: nothing stays unmatched)
    assert not np.array_equal(ref["track_id"], greedy["track_id"])  # the two rules part on these frames
    st, got, tails, _ = run_optimal(case)
    assert st == 0
    check_associate(got, ref, tails)


def test_optimal_associate_worked_example_chain_and_planted_ties(gpu_device):
    for spec in (WORKED, CHAIN, TIE_ONE_TRACK, TIE_TWO_TRACKS):
        case, ref = planted(spec, "optimal")
        st, got, tails, _ = run_optimal(case)
        assert st == 0
        check_associate(got, ref, tails)
        _, greedy = planted(spec, "greedy")                        # and the greedy entry is still the greedy rule on them
        st, got, tails, _ = run_associate(case)
        assert st == 0
        check_associate(got, greedy, tails)
    case, ref = planted(WORKED, "optimal")
    assert ref["track_id"][:, 1].tolist() == [1, 0] and ref["num_tracks"].tolist() == [2]
    case, _ = crafted_rows(3, 5, 3, 5, seed=2)
    case["n"][:] = 0                                               # nothing present
    st, got, tails, _ = run_optimal(case)
    assert st == 0 and all(tails.values()) and (got["track_id"] == -1).all() and (got["obj_state"] == 0).all()
    assert got["state_counts"].tolist() == [[15, 0, 0, 0, 0, 0]] * 3 and (got["num_tracks"] == 0).all()


def test_optimal_associate_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, _ = crafted_rows(3, 5, 2, 4, seed=8)
    off = torch.zeros(3 * 8 * 4 + 1, device="cuda")
    nan = float("nan")
    for kw, code in ((dict(what=None), -1), (dict(boxes=None), -1), (dict(n=None), -1), (dict(track_id=None), -1),
                     (dict(state_counts=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(S=0), -2), (dict(F=0), -2), (dict(A=0), -2),
                     (dict(R=9), -2), (dict(S=4, F=2, R=6), -2), (dict(iou_gate=1.0), -2), (dict(iou_gate=nan), -2),
                     (dict(appearance_weight=1.01), -2), (dict(birth_score=nan), -2), (dict(max_age=-1), -2),
                     (dict(boxes=Hh._p(off[1:])), -3)):
        st, got, tails, fill = run_optimal(case, **kw)
        assert st == code, kw
        assert all(tails.values()) and all((got[k] == fill[k]).all() for k in OUTPUTS), kw


# ---- 2. air_track_idf ---------------------------------------------------------------------------------------------------------------
POISON = 0x5A5A5A5A


def run_idf(case, tau=0.5, n_ids=None, **kw):
    from attend_infer_repeat_amd import hip as Hh
    T, S, F, G = case["T"], case["S"], case["F"], case["G"]
    R = S * F
    n_ids = F * T if n_ids is None else n_ids
    shapes = dict(overlap=(S, G, n_ids), seq_idf=(S, 4))
    bufs = {k: torch.full((int(np.prod(v)) + 64,), POISON, dtype=torch.int32, device="cuda") for k, v in shapes.items()}
    d = dict(boxes=dev_t(case["boxes"]), n=dev_t(case["n"].astype(np.int32)), ids=dev_t(case["ids"].astype(np.int32)), gt=dev_t(case["gt"]))
    p = Hh._p
    a = dict(boxes=p(d["boxes"]), n=p(d["n"]), ids=p(d["ids"]), gt=p(d["gt"]), tau=tau, T=T, G=G, S=S, F=F, R=R, n_ids=n_ids)
    a.update({k: p(bufs[k]) for k in shapes})
    a.update(kw)
    st = Hh.lib().air_track_idf(a["boxes"], a["n"], a["ids"], a["gt"], float(a["tau"]), a["T"], a["G"], a["S"], a["F"], a["R"],
                                a["n_ids"], a["overlap"], a["seq_idf"], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        got[k] = bufs[k][:n].view(shape).cpu().numpy()
        clean = clean and bool((bufs[k][n:] == POISON).all())
    return st, got, clean


@pytest.mark.parametrize("T,S,F,G,tau", [(3, 3, 5, 1, 0.5), (3, 3, 5, 8, 0.5), (6, 2, 17, 8, 0.3), (32, 1, 5, 8, 0.5), (1, 3, 2, 1, 0.0)])
def test_idf_is_the_reference(gpu_device, T, S, F, G, tau):
    case = identity_case(T, S, F, G, seed=T + S + F + G)
    want = track.reference_identity(case["boxes"], case["n"], case["ids"], case["gt"], F, tau)
    st, got, clean = run_idf(case, tau)
    assert st == 0 and clean
    assert not (got["overlap"] == POISON).any() and np.array_equal(got["overlap"], want["overlap"])     # every element written
    assert np.array_equal(got["seq_idf"], want["seq_idf"]), (got["seq_idf"], want["seq_idf"])
    print("seq_idf", want["seq_idf"].tolist())
    assert want["seq_idf"][:, 1].sum() > 0 and want["seq_idf"][:, 2].sum() > 0
    small = max(1, (F * T) // 2)                                   # ids from n_ids on are ignored
    want = track.reference_identity(case["boxes"], case["n"], case["ids"], case["gt"], F, tau, small)
    st, got, clean = run_idf(case, tau, small)
    assert st == 0 and clean and np.array_equal(got["overlap"], want["overlap"]) and np.array_equal(got["seq_idf"], want["seq_idf"])


def test_idf_with_a_fresh_id_in_every_frame(gpu_device):
    case = identity_case(1, 1, 40, 2, seed=7, fresh_ids=True)
    case["ids"][0] = np.arange(40)                                 # (every frame its own id: 40 columns, two passes of 32 ids)
    want = track.reference_identity(case["boxes"], case["n"], case["ids"], case["gt"], 40, 0.5)
    assert want["seq_idf"][0, 3] >= 10 and want["overlap"][0, :, 32:].any() and want["seq_idf"][0, 0] == 2 and want["overlap"].max() == 1
    st, got, clean = run_idf(case)
    assert st == 0 and clean and np.array_equal(got["overlap"], want["overlap"]) and np.array_equal(got["seq_idf"], want["seq_idf"])


def test_idf_argument_checks_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = identity_case(3, 2, 4, 2, seed=1)
    off = torch.zeros(2 * 8 * 4 + 1, device="cuda")
    for kw, code in ((dict(boxes=None), -1), (dict(ids=None), -1), (dict(gt=None), -1), (dict(overlap=None), -1), (dict(seq_idf=None), -1),
                     (dict(T=0), -2), (dict(T=33), -2), (dict(G=0), -2), (dict(G=9), -2), (dict(S=0), -2), (dict(F=0), -2), (dict(R=9), -2),
                     (dict(tau=-0.1), -2), (dict(tau=1.5), -2), (dict(tau=float("nan")), -2), (dict(n_ids=0), -2), (dict(n_ids=32768), -2),
                     (dict(gt=Hh._p(off[1:])), -3)):
        st, got, clean = run_idf(case, **kw)
        assert st == code, kw
        assert clean and all((got[k] == POISON).all() for k in got), kw


# ---- 3. SequenceTracker(matching="optimal") -------------------------------------------------------------------------------------------
def test_optimal_tracker_graph_replay_equals_eager_and_sequences_permute(gpu_device):
    S, F = 3, 5
    ocfg, eager, _ = make_tracker("rect_t5", S, F, birth_score=0.0, matching="optimal")
    _, graph, _ = make_tracker("rect_t5", S, F, capture=True, birth_score=0.0, matching="optimal")
    assert graph._graph is not None and eager._graph is None and graph.matching == "optimal"
    assert [e[2] for e in graph._plan] == ["air_track_associate_optimal", "air_track_owner"] and list(graph.segments) == ["associate", "owner"]
    assert graph.launch_count() == make_tracker("rect_t5", S, F, birth_score=0.0)[1].launch_count()
    keys = OUTPUTS + ("track_owner", "num_objects", "boxes", "owner")
    first = None
    for seed in (31, 32, 31):
        frames = frames_for(ocfg, S, F, seed).cuda()
        a, b = eager.track(frames), graph.track(frames)
        eager.synchronize(); graph.synchronize()
        for k in keys:
            assert torch.equal(a[k], b[k]), k
        first = first or {k: b[k].clone() for k in keys}
    assert all(torch.equal(first[k], b[k]) for k in keys) and first["num_tracks"].sum() > 0
    perm = [2, 0, 1]
    c = graph.track(frames[perm])
    graph.synchronize()
    rows = np.concatenate([np.arange(s * F, (s + 1) * F) for s in perm])
    for k in ("track_id", "obj_state", "affinity", "prev_frame", "prev_slot"):
        assert torch.equal(c[k], first[k][:, rows]), k
    for k in ("num_tracks", "track_first", "track_last", "track_length", "track_gaps", "state_counts"):
        assert torch.equal(c[k], first[k][perm]), k
    assert torch.equal(c["track_owner"], first["track_owner"][rows])
    graph.release_graphs()
    with pytest.raises(ValueError, match="matching must be one of"):
        make_tracker("rect_t5", S, F, matching="hungarian")


def test_optimal_tracker_is_the_reference_on_the_parse_and_greedy_is_unchanged(gpu_device):
    S, F = 3, 5
    ocfg, tk, pr = make_tracker("tiny", S, F, iou_gate=0.05, birth_score=0.0, matching="optimal")
    T, R = ocfg.max_steps, S * F
    frames = frames_for(ocfg, S, F, seed=21)
    counts = torch.from_numpy(np.random.default_rng(9).integers(0, T + 1, R).astype(np.int32)).cuda()
    out = tk.track(frames.cuda(), counts)
    tk.synchronize()
    rows = host_rows(out, T, R)
    assert rows["n"].max() > 0
    ref = track.reference_associate(rows["what"], rows["boxes"], rows["score"], rows["n"], F, iou_gate=0.05, birth_score=0.0,
                                    return_margins=True, matching="optimal")
    safe = ref["gate_margin"] >= MARGIN
    print("sequences inside the margin: %d of %d; tracks %s; states %s" % (safe.sum(), S, ref["num_tracks"].tolist(),
                                                                          ref["state_counts"].sum(0).tolist()))
    assert safe.sum() >= S - 1 and ref["num_tracks"].sum() > 0
    in_rows = np.repeat(safe, F)
    for k in OUTPUTS:
        g, want = out[k].cpu().numpy(), ref[k]
        g, want = (g[:, in_rows], want[:, in_rows]) if k in OUTPUTS[:5] else (g[safe], want[safe])
        assert np.array_equal(bits(g), bits(want)) if k == "affinity" else np.array_equal(g, want), k
    assert np.array_equal(out["track_owner"].cpu().numpy(), owner_reference(out["owner"].cpu().numpy(), out["track_id"].cpu().numpy(), T))
    # matching="greedy" is the tracker built without the argument, bit for bit
    _, plain, _ = make_tracker("tiny", S, F, iou_gate=0.05, birth_score=0.0)
    _, greedy, _ = make_tracker("tiny", S, F, iou_gate=0.05, birth_score=0.0, matching="greedy")
    assert [e[2] for e in plain._plan] == [e[2] for e in greedy._plan] == ["air_track_associate", "air_track_owner"]
    a, b = plain.track(frames.cuda(), counts), greedy.track(frames.cuda(), counts)
    plain.synchronize(); greedy.synchronize()
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8) if t.is_floating_point() else t
    assert set(a) == set(b) and all(torch.equal(raw(a[k]), raw(b[k])) for k in OUTPUTS + ("track_owner",))


# ---- 4. scores and totals -------------------------------------------------------------------------------------------------------------
def test_identity_totals_accumulate_and_reset_and_summary_is_unchanged(gpu_device):
    S, F, G = 3, 5, 2
    ocfg, tk, pr = make_tracker("rect_t5", S, F, capture=True, birth_score=0.0, matching="optimal")
    T, R = ocfg.max_steps, S * F
    out = tk.track(frames_for(ocfg, S, F, 31).cuda())
    tk.synchronize()
    rows = host_rows(out, T, R)
    ids = out["track_id"].cpu().numpy()
    gt = moving_gt(dict(boxes=rows["boxes"], n=rows["n"], T=T, S=S, F=F), np.random.default_rng(1), G).reshape(S, F, G, 4)
    want = track.reference_score(rows["boxes"], rows["n"], ids, gt, F, 0.5)
    idf = track.reference_identity(rows["boxes"], rows["n"], ids, gt, F, 0.5)
    plain = tk.score(torch.from_numpy(gt), accumulate=False)      # an entry without identity: one launch, today's keys
    assert set(plain) == {"seq_counts", "seq_iou", "gt_match", "totals_i", "totals_f"} and list(tk._score) == [(G, 0.5)]
    assert [e[2] for e in tk._score[(G, 0.5)]["plan"]] == ["air_track_score"]
    before = tk.summary()
    a = tk.score(torch.from_numpy(gt), accumulate=False, identity=True)
    tk.synchronize()
    assert set(a) == set(plain) | {"seq_idf", "idf_overlap", "totals_idf"} and list(tk._score) == [(G, 0.5), (G, 0.5, "idf")]
    entry = tk._score[(G, 0.5, "idf")]
    assert [e[2] for e in entry["plan"]] == ["air_track_score", "air_track_idf"] and entry["graph"] is not None
    assert np.array_equal(a["seq_counts"].cpu().numpy(), want["seq_counts"]) and np.array_equal(a["gt_match"].cpu().numpy(), want["gt_match"])
    assert np.array_equal(a["seq_idf"].cpu().numpy(), idf["seq_idf"]) and np.array_equal(a["idf_overlap"].cpu().numpy(), idf["overlap"])
    assert a["totals_idf"].dtype == torch.int64 and a["totals_idf"].tolist() == idf["seq_idf"].sum(0).tolist()
    same = lambda p, q: set(p) == set(q) and all(p[k] == q[k] or (np.isnan(p[k]) and np.isnan(q[k])) for k in p)
    once = tk.summary()                                            # summary() is what it was: mot_summary of the same sums
    assert same(once, before) and same(once, track.mot_summary(want["seq_counts"].sum(0), float(a["totals_f"][0])))
    assert same(tk.identity_summary(), track.idf_summary(idf["seq_idf"].sum(0))) and idf["seq_idf"][:, 1].sum() == once["gt"] > 0
    tk.score(torch.from_numpy(gt).cuda(), accumulate=True, identity=True)
    twice = tk.identity_summary()
    for k in ("idtp", "idfp", "idfn", "gt_frames", "hyp_frames"):
        assert twice[k] == 2 * track.idf_summary(idf["seq_idf"].sum(0))[k], k
    assert tk.summary()["gt"] == 2 * once["gt"]
    tk.score(torch.from_numpy(gt), accumulate=True)                # without identity: totals_idf stays
    assert tk.identity_summary() == twice and tk.summary()["gt"] == 3 * once["gt"]
    tk.reset()
    empty = tk.identity_summary()
    assert empty["gt_frames"] == empty["idtp"] == 0 and np.isnan(empty["idf1"]) and tk.summary()["gt"] == 0
    for tau in (0.1, 0.2, 0.3, 0.4):                               # the cap of four entries
        tk.score(torch.from_numpy(gt), tau=tau, accumulate=False, identity=True)
    assert len(tk._score) == 4 and all(k[-1] == "idf" for k in tk._score)
    tk.release_graphs()


def test_the_smoothers_completed_table_is_scored_with_identity(gpu_device):
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    S, F, G = 2, 4, 2
    ocfg, tk, pr = make_tracker("rect_t5", S, F, birth_score=0.0, matching="optimal")
    sm = TrajectorySmoother(tk, horizon=2)
    out = sm.track(frames_for(ocfg, S, F, 31).cuda())
    sm.synchronize()
    C, R = sm.C, S * F
    boxes, n, ids = (out[k].cpu().numpy() for k in ("sm_boxes", "sm_count", "sm_id"))
    gt = moving_gt(dict(boxes=boxes, n=n, T=C, S=S, F=F), np.random.default_rng(2), G)
    a = sm.score(torch.from_numpy(gt), accumulate=False, identity=True)
    sm.synchronize()
    want = track.reference_identity(boxes, n, ids, gt, F, 0.5, F * ocfg.max_steps)
    assert tuple(a["idf_overlap"].shape) == (S, G, F * ocfg.max_steps)
    assert np.array_equal(a["seq_idf"].cpu().numpy(), want["seq_idf"]) and np.array_equal(a["idf_overlap"].cpu().numpy(), want["overlap"])
    assert want["seq_idf"][:, 2].sum() > 0 and sm.identity_summary() == track.idf_summary(want["seq_idf"].sum(0))
    assert np.array_equal(a["seq_counts"].cpu().numpy(), track.reference_score(boxes, n, ids, gt, F, 0.5)["seq_counts"])
    fboxes, fn, fids = (out[k].cpu().numpy() for k in ("fc_boxes", "fc_count", "fc_id"))
    fgt = moving_gt(dict(boxes=fboxes, n=fn, T=C, S=S, F=2), np.random.default_rng(3), G)
    b = sm.score_forecast(torch.from_numpy(fgt), identity=True)
    sm.synchronize()
    want = track.reference_identity(fboxes, fn, fids, fgt, 2, 0.5, F * ocfg.max_steps)
    assert np.array_equal(b["seq_idf"].cpu().numpy(), want["seq_idf"]) and "totals_idf" not in b
    assert set(sm.score(torch.from_numpy(gt), accumulate=False)) == {"seq_counts", "seq_iou", "gt_match", "totals_i", "totals_f"}


def test_score_track_optimal_with_identity_does_not_disturb_training(gpu_device):
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    B, S, F, T = 8, 2, 4, 3
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    d = procedural_moving_mnist(S, F, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    before, obs_before = _train_state(air._engine), air.obs
    scores, tracker = air.score_track(frames, d["boxes"], accumulate=False, matching="optimal", identity=True)
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air.obs is obs_before and air._engine.global_step == 2
    assert tracker.matching == "optimal" and tracker is air.tracker(S, F, matching="optimal") and tracker is not air.tracker(S, F)
    assert air.tracker(S, F) is air.tracker(S, F, matching="greedy") and len(air._trackers) == 2
    R, G = S * F, d["boxes"].shape[-2]
    assert tuple(scores["seq_idf"].shape) == (S, 4) and tuple(scores["idf_overlap"].shape) == (S, G, F * T)
    out = air.tracked
    want = track.reference_identity(out["boxes"].cpu().numpy(), out["num_objects"].cpu().numpy(), out["track_id"].cpu().numpy(),
                                    d["boxes"], F, 0.5)
    assert np.array_equal(scores["seq_idf"].cpu().numpy(), want["seq_idf"])
    fig, mot = tracker.identity_summary(), tracker.summary()
    assert fig["gt_frames"] == mot["gt"] == int((d["boxes"][..., 2] > 0).sum()) and fig["idtp"] + fig["idfn"] == fig["gt_frames"]
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params) and torch.equal(air._engine.rng_state, twin._engine.rng_state)
    with pytest.raises(ValueError, match="matching must be one of"):
        air.track(frames, matching="best")
    frames_pred, res = air.predict_frames(frames, 2, matching="optimal")
    assert tuple(frames_pred.shape) == (S, 2, 50, 50) and air.tracker(S, F, smooth=dict(horizon=2), matching="optimal").matching == "optimal"
