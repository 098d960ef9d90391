"""GPU tests of the trajectory smoother (attend_infer_repeat_amd/trajectory.py, csrc/trajectory_kernels.hip): air_track_smooth and
air_track_fill on planted tracker outputs against trajectory.reference_smooth, then TrajectorySmoother behind the providers, its
scores, the predicted frames and the model's surface.

Bars.  EVERY output element is compared exactly: the integers as integers, the floats by their bits (a NaN by its position).  The
rule is float64 with only + - * / in one stated order, contraction off on the device, so numpy float64 and the kernel round every
operation alike; the fp32 outputs are that float64 rounded once, or fp32 operations in air_parse_objects' order."""
import numpy as np
import pytest
import torch

from test_parse import SENTINEL_F, SENTINEL_I, _mnist_air, e2e_case, make_parser
from trajectory_cases import (IMG, PLANTED, drifting_case, full_table_case, jumping_case, planted_sequences, reference,
                              rows_from_objects, with_tracker)

from attend_infer_repeat_amd import track, trajectory
from attend_infer_repeat_amd.trajectory import ABSENT, FILLED, FORECAST, OBSERVED

pytestmark = pytest.mark.gpu

TAIL = 64
dev_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
TABLE_DTYPES = dict(where=torch.float32, boxes=torch.float32, id=torch.int32, state=torch.int8, src_frame=torch.int32,
                    src_slot=torch.int32, velocity=torch.float32, count=torch.int32)
ORDER = ("where", "boxes", "id", "state", "src_frame", "src_slot", "velocity", "count")      # the entry's order per table


def raw_bits(a):
    """integers as they are; floats by their bits, every NaN as ONE value: the positions of the NaNs are compared, their sign and
    payload are not (IEEE 754 leaves the NaN an operation such as inf - inf makes to the implementation; x86 and gfx950 differ)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def sentinel(shape, dtype, tail=TAIL, offset=0):
    """a sentinel-filled flat buffer of offset + prod(shape) + tail elements; returns (flat, the view behind `offset`, fill)"""
    fill = SENTINEL_F if dtype.is_floating_point else (99 if dtype == torch.int8 else SENTINEL_I)
    flat = torch.full((offset + int(np.prod(shape)) + tail,), fill, dtype=dtype, device="cuda")
    return flat, flat[offset:], fill


def table_shapes(C, N):
    return dict(where=(C, N, 4), boxes=(C, N, 4), id=(C, N), state=(C, N), src_frame=(C, N), src_slot=(C, N), velocity=(C, N, 2),
                count=(N,))


def run_smooth(case, horizon=0, noise=None, **kw):
    """air_track_smooth alone (current stream) on the planted tracker outputs of a case; every output and a tail behind it start as
    a sentinel fill.  Returns status, {name: host array}, whether every tail is untouched, {name: fill}"""
    from attend_infer_repeat_amd import hip as Hh
    L, p = Hh.lib(), Hh._p
    T, S, F, R, max_age = case["T"], case["S"], case["F"], case["R"], case["max_age"]
    C, Hz, N = trajectory.completed_rows(T, max_age), horizon, S * horizon
    noise = dict(trajectory.DEFAULTS, **(noise or {}))
    d = dict(where=dev_t(case["where"]), n=dev_t(case["n"].astype(np.int32)), track_id=dev_t(case["track_id"]),
             num_tracks=dev_t(case["num_tracks"]), track_first=dev_t(case["track_first"]), track_last=dev_t(case["track_last"]))
    ws_bytes = int(L.air_track_smooth_workspace_bytes(C, R))
    ws = torch.zeros(max(ws_bytes // 8, 1), dtype=torch.float64, device="cuda")
    bufs = {}
    for pre, cols in (("sm_", R), ("fc_", N)):
        if cols:
            bufs.update({pre + k: sentinel(shp, TABLE_DTYPES[k]) + (shp,) for k, shp in table_shapes(C, cols).items()})
    bufs["sm_counts"] = sentinel((S, 3), torch.int32) + ((S, 3),)
    a = dict(where=p(d["where"]), n=p(d["n"]), track_id=p(d["track_id"]), num_tracks=p(d["num_tracks"]), track_first=p(d["track_first"]),
             track_last=p(d["track_last"]), T=T, S=S, F=F, R=R, C=C, Hz=Hz, max_age=max_age, H=case["img"][0], W=case["img"][1],
             q_shift=noise["process_noise"][0], q_scale=noise["process_noise"][1], r=noise["measurement_noise"],
             velocity_var=noise["velocity_var"], ws=p(ws), ws_bytes=ws_bytes)
    a.update({k: p(v[1]) for k, v in bufs.items()})
    for k in ORDER:
        a.setdefault("fc_" + k, None)
    a.update(kw)
    st = L.air_track_smooth(a["where"], a["n"], a["track_id"], a["num_tracks"], a["track_first"], a["track_last"], a["T"], a["S"], a["F"],
                            a["R"], a["C"], a["Hz"], a["max_age"], a["H"], a["W"], float(a["q_shift"]), float(a["q_scale"]), float(a["r"]),
                            float(a["velocity_var"]), a["ws"], a["ws_bytes"], *[a["sm_" + k] for k in ORDER], a["sm_counts"],
                            *[a["fc_" + k] for k in ORDER], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, (flat, view, fill, shp) in bufs.items():
        n = int(np.prod(shp))
        got[k] = view[:n].view(shp).cpu().numpy()
        clean = clean and bool((view[n:] == fill).all())
    return st, got, clean, {k: v[2] for k, v in bufs.items()}, bufs


def run_fill(case, table, per_seq, what_offset=0):
    """air_track_fill alone on a table's device buffers (state, src_frame, src_slot as air_track_smooth left them); the provider's
    what buffer may start `what_offset` floats past an aligned address"""
    from attend_infer_repeat_amd import hip as Hh
    L, p = Hh.lib(), Hh._p
    T, F, R, A, G = case["T"], case["F"], case["R"], case["A"], case["G"]
    C, N = table["state"][3]
    what_flat = torch.zeros(what_offset + T * R * A, device="cuda")
    what_flat[what_offset:] = dev_t(case["what"]).reshape(-1)
    glimpse, score = dev_t(case["glimpse"]), dev_t(case["score"])
    outs = {k: sentinel(shp, torch.float32) + (shp,) for k, shp in (("what", (C, N, A)), ("glimpse", (C, N, G)), ("score", (C, N)))}
    st = L.air_track_fill(p(what_flat[what_offset:]), p(glimpse), p(score), p(table["state"][1]), p(table["src_frame"][1]),
                          p(table["src_slot"][1]), T, F, R, C, N, per_seq, A, G, p(outs["what"][1]), p(outs["glimpse"][1]),
                          p(outs["score"][1]), Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k, (flat, view, fill, shp) in outs.items():
        n = int(np.prod(shp))
        got[k] = view[:n].view(shp).cpu().numpy()
        clean = clean and bool((view[n:] == fill).all())
    return st, got, clean


def check_tables(got, ref, horizon):
    for pre in ("sm_",) + (("fc_",) if horizon else ()):
        for k in ORDER:
            g, w = got[pre + k], ref[pre + k]
            assert g.dtype == w.dtype and g.shape == w.shape, (pre + k, g.dtype, w.dtype, g.shape, w.shape)
            assert np.array_equal(raw_bits(g), raw_bits(w)), (pre + k, np.argwhere(raw_bits(g) != raw_bits(w))[:4])
    assert np.array_equal(got["sm_counts"], ref["sm_counts"])


def smooth_and_fill_against_the_reference(case, horizon, noise=None, what_offset=0):
    ref = reference(case, horizon, **(noise or {}))
    st, got, clean, _, bufs = run_smooth(case, horizon, noise)
    assert st == 0 and clean
    check_tables(got, ref, horizon)
    for pre, per_seq in (("sm_", case["F"]),) + ((("fc_", horizon),) if horizon else ()):
        table = {k: bufs[pre + k] for k in ("state", "src_frame", "src_slot")}
        st, filled, clean = run_fill(case, table, per_seq, what_offset)
        assert st == 0 and clean
        for k in ("what", "glimpse", "score"):
            assert np.array_equal(raw_bits(filled[k]), raw_bits(ref[pre + k])), pre + k
    return ref


# ---- 1. the two entries on planted tracker outputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 5, 8])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("max_age,horizon,A,G,off", [(1, 0, 5, 16, 0), (2, 3, 8, 7, 0), (0, 3, 4, 16, 1)])
def test_smooth_and_fill_are_the_reference(gpu_device, F, S, max_age, horizon, A, G, off):
    """T = 3; sequence boundaries, gaps at max_age 1 and 2, none at 0, a track born in the last frame; A and G a multiple of 4 and
    not, a `what` buffer one float past alignment (the 4-byte copy path)"""
    case = drifting_case(3, F, S, max_age, A=A, G=G, seed=10 * F + S + max_age, dropout=0.3)
    noise = dict(process_noise=(2e-4, 5e-5), measurement_noise=3e-4, velocity_var=0.05) if horizon else None
    ref = smooth_and_fill_against_the_reference(case, horizon, noise, off)
    filled = int(ref["sm_counts"][:, FILLED].sum())
    print("F=%d S=%d max_age=%d: tracks %s, filled rows %d" % (F, S, max_age, case["num_tracks"].tolist(), filled))
    assert max_age > 0 or filled == 0                              # max_age = 0: no FILLED row can occur
    if F >= 2:
        born_last = [(s, i) for s in range(S) for i in range(int(case["num_tracks"][s])) if case["track_first"][s, i] == F - 1]
        assert born_last
    if F == 8 and max_age > 0:
        assert filled > 0


def test_full_table_and_more_ids_than_lanes(gpu_device):
    ref = smooth_and_fill_against_the_reference(full_table_case(), 3)      # T = 32, F = 2: 32 live tracks, C = 32
    assert ref["sm_id"].shape[0] == 32 and (ref["sm_count"] == 32).all() and (ref["fc_count"] == 32).all()
    case = jumping_case()                                          # T = 3, F = 24: 72 ids of one sighting, two passes of lanes
    assert int(case["num_tracks"][0]) == 72 > 64
    ref = smooth_and_fill_against_the_reference(case, 3)
    assert (ref["sm_state"][:3] == OBSERVED).all() and (ref["sm_velocity"] == 0).all()
    churn = drifting_case(32, 6, 1, 1, A=4, G=4, seed=7, dropout=0.35)      # 52 ids over a full live table, tracks dying and reborn
    smooth_and_fill_against_the_reference(churn, 0)


def test_non_finite_sightings_nan_positions_too(gpu_device):
    case, _, _, _ = planted_sequences()
    j = int(np.nonzero(case["track_id"][:, 3] == 0)[0][0])
    case["where"][j, 3, 1] = np.nan
    j = int(np.nonzero(case["track_id"][:, 9] == 1)[0][0])
    case["where"][j, 9, 2] = np.inf                                # inf - inf further on: NaN
    ref = smooth_and_fill_against_the_reference(case, 2)
    assert np.isnan(ref["sm_where"]).any() and np.isfinite(ref["sm_where"][..., 0][ref["sm_id"] == 0]).all()


def test_a_refused_call_writes_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = drifting_case(3, 5, 2, 1, seed=3)
    nan = float("nan")
    off = torch.zeros(3 * 10 * 4 + 1, device="cuda")
    for kw, code in ((dict(q_shift=0.0), -2), (dict(q_scale=-1e-4), -2), (dict(q_shift=nan), -2), (dict(r=0.0), -2), (dict(r=nan), -2),
                     (dict(velocity_var=-1e-9), -2), (dict(velocity_var=nan), -2), (dict(Hz=17), -2), (dict(Hz=-1), -2), (dict(C=5), -2),
                     (dict(C=7), -2), (dict(T=0), -2), (dict(T=33), -2), (dict(R=11), -2), (dict(S=0), -2), (dict(F=0), -2),
                     (dict(max_age=-1), -2), (dict(where=None), -1), (dict(track_id=None), -1), (dict(sm_where=None), -1),
                     (dict(fc_boxes=None), -1), (dict(ws=None), -1), (dict(ws_bytes=8), -4), (dict(where=Hh._p(off[1:])), -3),
                     # outside the supported noise domain (r = 4e-4): velocity_var / r > 1e6, q / r > 1e15, q / r < 1e-29, r out of range
                     (dict(velocity_var=1e6), -2), (dict(velocity_var=401.0), -2), (dict(q_shift=4.1e11), -2), (dict(q_scale=1e-33), -2),
                     (dict(q_shift=1.0, q_scale=1.0, r=3e-17, velocity_var=0.0), -2),
                     (dict(q_shift=1e-300, q_scale=1e-300, r=1e-300, velocity_var=0.0), -2),
                     (dict(q_shift=1e140, q_scale=1e140, r=1e140, velocity_var=1e140), -2)):
        st, got, clean, fill, _ = run_smooth(case, 3, **kw)
        assert st == code, (kw, st)
        assert clean and all((got[k] == fill[k]).all() for k in got), kw
    big = dict(case, T=32, F=1024, S=1, R=1024)                    # 1024 * 32 ids do not fit the tracker's int16 (refused before any read)
    st, got, clean, fill, _ = run_smooth(big, 0, C=32)
    assert st == -2


def test_first_run_and_graph_replay_give_identical_bits(gpu_device):
    S, F, Hz = 3, 5, 3
    ocfg, sm, tk, pr = make_smoother("rect_t5", S, F, horizon=Hz)
    frames = frames_for(ocfg, S, F, 31).cuda()
    keys = [k for k in sm.track(frames) if k.startswith(("sm_", "fc_")) or k == "frames_pred"]
    first = {k: v.clone() for k, v in sm.track(frames).items() if k in keys}
    sm.synchronize()
    for s in (pr, tk, sm):
        s.capture()
    assert sm._graph is not None and set(sm.segments) == {"smooth", "fill", "readout", "fill_forecast", "readout_forecast"}
    sm.track(frames_for(ocfg, S, F, 32).cuda())                    # something else in between
    again = sm.track(frames)
    sm.synchronize()
    raw = lambda t: t.contiguous().view(torch.uint8) if t.is_floating_point() else t
    for k in keys:
        assert torch.equal(raw(first[k]), raw(again[k])), k
    assert int(first["sm_count"].sum()) > 0 and sm.launch_count()["track_smooth"] == 1
    sm.release_graphs(); tk.release_graphs()


# ---- 2. TrajectorySmoother --------------------------------------------------------------------------------------------------------------
def make_smoother(name, S, F, provider="scene", horizon=0, capture=False, max_age=1, **kw):
    from attend_infer_repeat_amd.temporal import TemporalProposer
    from attend_infer_repeat_amd.track import SequenceTracker
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    ocfg, _, params, _ = e2e_case(name)
    ps = make_parser(ocfg, S * F, params)
    pr = ps if provider == "scene" else TemporalProposer(ps, F, 1, 1)
    tk = SequenceTracker(pr, F, iou_gate=0.05, birth_score=0.0, max_age=max_age)        # (an untrained model's scores are low)
    sm = TrajectorySmoother(tk, horizon=horizon, **kw)
    if capture:
        for s in ([ps] if pr is ps else [ps, pr]) + [tk, sm]:
            s.capture()
    return ocfg, sm, tk, pr


def frames_for(ocfg, S, F, seed):
    from test_track import frames_for as base
    return base(ocfg, S, F, seed)


def host_case(out, sm, tk):
    """the provider's and the tracker's device buffers of the latest call, as a case of trajectory_cases"""
    np_ = lambda t: t.detach().cpu().numpy()
    T, R = tk.T, tk.R
    return dict(where=np_(sm._rows["where"]).reshape(T, R, 4), what=np_(sm._rows["what"]).reshape(T, R, -1),
                glimpse=np_(sm._rows["glimpse"]).reshape(T, R, -1), score=np_(sm.provider.score), n=np_(sm.provider.num_objects),
                track_id=np_(tk.track_id), num_tracks=np_(tk.num_tracks), track_first=np_(tk.track_first), track_last=np_(tk.track_last),
                T=T, R=R, F=tk.F, S=tk.S, max_age=tk.max_age, img=tk.img_size)


@pytest.mark.parametrize("provider,max_age", [("scene", 1), ("temporal", 2)])
def test_smoother_only_reads_and_is_the_reference(gpu_device, provider, max_age):
    S, F, Hz = 3, 5, 2
    ocfg, sm, tk, pr = make_smoother("tiny", S, F, provider, horizon=Hz, capture=True, max_age=max_age)
    T, R = ocfg.max_steps, S * F
    assert (sm.T, sm.C, sm.R, sm.window_T, sm.engine) == (T * (max_age + 1),) * 2 + (R, T, pr.engine)
    frames = frames_for(ocfg, S, F, seed=21).cuda()
    counts = torch.from_numpy(np.random.default_rng(9).integers(0, T + 1, R).astype(np.int32)).cuda()
    base = tk.track(frames, counts)
    tk.synchronize()
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8).clone() if t.is_floating_point() else t.clone()
    watched = {k: v for k, v in base.items() if torch.is_tensor(v)}
    watched.update({"rows_" + k: v for k, v in sm._rows.items()})
    before = {k: raw(v) for k, v in watched.items()}
    out = sm.run(base)
    sm.synchronize()
    for k, v in watched.items():                                   # the provider's and the tracker's buffers: unchanged bit for bit
        assert torch.equal(before[k], raw(v)), k
    case = host_case(out, sm, tk)
    ref = reference(case, Hz)
    got = {k: out[k].cpu().numpy() for k in ref if k in out and k != "sm_glimpse" and k != "fc_glimpse"}
    for k in got:
        assert np.array_equal(raw_bits(got[k]), raw_bits(ref[k])), k
    for pre in ("sm_", "fc_"):
        assert np.array_equal(raw_bits(out[pre + "glimpse"].cpu().numpy().reshape(ref[pre + "glimpse"].shape)), raw_bits(ref[pre + "glimpse"]))
    assert len(got) == 2 * 10 + 1
    assert int(ref["sm_count"].sum()) > 0 or provider == "temporal"       # (the subset search may empty every frame of a random model)
    # the read-out: air_parse_objects' boxes are sm_boxes' bits, the counts and ids go through
    n = ref["sm_count"]
    live = np.arange(sm.C)[:, None] < n[None, :]
    assert torch.equal(sm.num_objects.cpu(), torch.from_numpy(n)) and np.array_equal(sm.presence.cpu().numpy() > 0.5, live)
    assert np.array_equal(raw_bits(sm.boxes.cpu().numpy()[live]), raw_bits(ref["sm_boxes"][live]))
    assert np.array_equal(raw_bits(sm.completed.score.cpu().numpy()[live]), raw_bits(ref["sm_score"][live]))
    assert np.array_equal(out["sm_obj_step"].cpu().numpy()[:n.sum()], ref["sm_id"].T[live.T])
    assert out["sm_owner"].shape == (R,) + tuple(ocfg.img_size) and int(out["sm_owner"].max()) < sm.C
    assert tuple(out["frames_pred"].shape) == (S, Hz) + tuple(ocfg.img_size)
    print("%s: completed rows %d of them filled %d, forecast rows %d" % (provider, n.sum(), ref["sm_counts"][:, FILLED].sum(),
                                                                      ref["fc_count"].sum()))
    sm.release_graphs(); tk.release_graphs()


def test_score_on_the_completed_table_is_the_reference_and_scorer_binds(gpu_device):
    from attend_infer_repeat_amd.score import ParseScorer
    S, F, G = 3, 5, 2
    ocfg, sm, tk, pr = make_smoother("rect_t5", S, F, horizon=2, capture=True)
    out = sm.track(frames_for(ocfg, S, F, 31).cuda())
    sm.synchronize()
    boxes, n, ids = (out[k].cpu().numpy() for k in ("sm_boxes", "sm_count", "sm_id"))
    rng = np.random.default_rng(1)
    gt = np.zeros((S * F, G, 4), np.float32)
    for r in range(S * F):
        for g in range(G):
            if n[r] and rng.uniform() < 0.8:
                gt[r, g] = boxes[int(rng.integers(n[r])), r] + rng.normal(size=4).astype(np.float32) * 0.5
    want = track.reference_score(boxes, n, ids, gt, F, 0.5)
    a = sm.score(torch.from_numpy(gt.reshape(S, F, G, 4)), accumulate=False)
    sm.synchronize()
    assert np.array_equal(a["seq_counts"].cpu().numpy(), want["seq_counts"]) and np.array_equal(a["gt_match"].cpu().numpy(), want["gt_match"])
    assert np.allclose(a["seq_iou"].cpu().numpy(), want["seq_iou"], rtol=1e-12, atol=0)      # (test_track.py's bar for this sum)
    once = sm.summary()
    assert once["gt"] == int((gt[..., 2] > 0).sum()) > 0
    assert once == track.mot_summary(want["seq_counts"].sum(0), float(a["totals_f"][0])) or np.isnan(once["motp"])
    sm.score(torch.from_numpy(gt).cuda(), accumulate=True)
    assert sm.summary()["gt"] == 2 * once["gt"] and tk.summary()["gt"] == 0      # totals of its own
    sm.reset()
    assert sm.summary()["gt"] == 0
    fb, fn, fi = (out[k].cpu().numpy() for k in ("fc_boxes", "fc_count", "fc_id"))
    gtf = np.zeros((S * 2, G, 4), np.float32)
    gtf[:, 0] = np.where(fn[:, None] > 0, fb[0], 0)
    wf = track.reference_score(fb, fn, fi, gtf, 2, 0.5)
    f = sm.score_forecast(torch.from_numpy(gtf))
    assert np.array_equal(f["seq_counts"].cpu().numpy(), wf["seq_counts"]) and np.array_equal(f["gt_match"].cpu().numpy(), wf["gt_match"])
    with pytest.raises(ValueError, match="gt_boxes"):
        sm.score(torch.zeros(S * F + 1, G, 4))
    sc = ParseScorer(sm.completed, G)                              # the provider surface: the completed frames
    assert (sc.T, sc.R) == (sm.C, S * F)
    sm.release_graphs(); tk.release_graphs()


def test_refusals(gpu_device):
    from attend_infer_repeat_amd.track import SequenceTracker
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    ocfg, _, params, _ = e2e_case("tiny")
    tk = SequenceTracker(make_parser(ocfg, 10, params), 5)
    for kw, word in ((dict(horizon=17), "horizon"), (dict(process_noise=(0.0, 1.0)), "process_noise"), (dict(measurement_noise=-1.0), "measurement_noise"),
                     (dict(velocity_var=float("nan")), "velocity_var")):
        with pytest.raises(ValueError, match=word):
            TrajectorySmoother(tk, **kw)
    with pytest.raises(ValueError, match="horizon"):
        TrajectorySmoother(tk).score_forecast(torch.zeros(2, 1, 1, 4))


# ---- 3. the planted sequences through the module and the model ------------------------------------------------------------------------
def plant(provider, case):
    """overwrite the provider's device buffers with the rows of a planted case (what a parse of such frames would have left)"""
    from attend_infer_repeat_amd.tile import _provider_rows
    rows = _provider_rows(provider)
    torch.cuda.synchronize()
    for buf, k in ((rows["what"], "what"), (rows["where"], "where"), (rows["glimpse"], "glimpse"), (provider.boxes, "boxes"),
                   (provider.score, "score"), (provider.num_objects, "n")):
        buf.view(-1).copy_(torch.from_numpy(np.ascontiguousarray(case[k])).reshape(-1).to(buf.dtype))
    torch.cuda.synchronize()


def test_predict_frames_and_the_planted_sequences_on_the_model(gpu_device):
    """AIRonMNIST.score_track(smooth=) and predict_frames with the planted rows in the provider's buffers (its parse() is wrapped: the
    model is untrained): one miss per planted gap on the raw table, none on the completed one, as on the host; the predicted frames
    are air_parse_render run by hand on the forecast rows, bit for bit; smooth=None returns today's result object for object"""
    from attend_infer_repeat_amd import hip as Hh
    S, F, K, Hz = PLANTED["S"], PLANTED["F"], PLANTED["K"], PLANTED["HZ"]
    air, ts, x, y = _mnist_air(8)
    ts()
    case, gt, gt_future, gaps = planted_sequences(A=50, G=400)
    frames = torch.zeros(S, F, 50, 50).cuda()
    plain = air.track(frames)
    assert plain is air.tracked and not any(k.startswith(("sm_", "fc_")) for k in plain) and len(air._trackers) == 1
    assert air.track(frames, smooth=None) is not None and len(air._trackers) == 1 and air.tracker(S, F) is air.tracker(S, F, smooth=None)
    same = lambda a, b: a.data_ptr() == b.data_ptr() and a.shape == b.shape if torch.is_tensor(a) else a == b
    assert set(air.track(frames, smooth=None)) == set(plain) and all(same(air.tracked[k], plain[k]) for k in plain)
    spec = dict(horizon=Hz)
    sm = air.trajectory_smoother(S, F, spec)
    assert sm is air.trajectory_smoother(S, F, dict(horizon=Hz)) and sm.tracker is air.tracker(S, F, smooth=spec) and len(air._trackers) == 2
    assert sm._graph is not None and sm.tracker is not air.tracker(S, F) and sm.horizon == Hz
    inner = sm.provider.parse

    def planted_parse(*args, **kwargs):
        base = inner(*args, **kwargs)
        plant(sm.provider, case)
        return base

    sm.provider.parse = planted_parse
    scores, tk = air.score_track(frames, gt, tau=PLANTED["TAU"], accumulate=False, smooth=spec)
    assert tk is sm.tracker and air.track_smoother is sm
    raw, done = tk.summary(), sm.summary()
    print("planted on the model: raw misses %d mota %.4f; completed misses %d mota %.4f" % (raw["misses"], raw["mota"], done["misses"],
                                                                                          done["mota"]))
    assert raw["misses"] == gaps and done["misses"] == 0 and raw["gt"] == done["gt"] == S * F * K
    assert raw["false_positives"] == done["false_positives"] == 0 and done["mota"] == 1.0 > raw["mota"]
    ref = reference(case, Hz)
    want = track.reference_score(ref["sm_boxes"], ref["sm_count"], ref["sm_id"], gt, F, PLANTED["TAU"])
    assert np.array_equal(scores["completed"]["seq_counts"].cpu().numpy(), want["seq_counts"])
    ahead = sm.score_forecast(torch.from_numpy(gt_future), PLANTED["TAU"])["seq_counts"].cpu().numpy()
    assert ahead[:, track.COUNTS.index("misses")].sum() == 0 and ahead[:, track.COUNTS.index("matches")].sum() == S * Hz * K
    pred, out = air.predict_frames(frames, Hz)
    assert tuple(pred.shape) == (S, Hz, 50, 50) and out is air.tracked and pred.data_ptr() == out["frames_pred"].data_ptr()
    assert np.array_equal(raw_bits(out["fc_where"].cpu().numpy()), raw_bits(ref["fc_where"]))
    # air_parse_render by hand on the forecast rows
    cfg, L, p = sm.engine.cfg, Hh.lib(), Hh._p
    N, C = S * Hz, sm.C
    rec, owner = torch.full((N, 50, 50), SENTINEL_F, device="cuda"), torch.zeros((N, 50, 50), dtype=torch.int8, device="cuda")
    area = torch.zeros((C, N), dtype=torch.int32, device="cuda")
    presence = (torch.arange(C, device="cuda")[:, None] < out["fc_count"][None, :]).float().contiguous()
    torch.cuda.synchronize()
    st = L.air_parse_render(p(out["fc_glimpse"]), p(out["fc_where"]), p(presence), None, float(cfg.output_multiplier), float(cfg.output_std),
                            sm.mask_threshold, C, N, 50, 50, cfg.crop_size[0], cfg.crop_size[1], int(L.air_canvas_unroll_bands(N, 50)),
                            p(rec), None, p(owner), p(area), None, Hh._stream())
    torch.cuda.synchronize()
    assert st == 0 and torch.equal(rec.view(torch.int32), pred.reshape(N, 50, 50).view(torch.int32)) and float(pred.abs().max()) > 0
    assert torch.equal(owner, out["fc_owner"])
    with pytest.raises(ValueError, match="horizon"):
        air.predict_frames(frames, 0)
    with pytest.raises(ValueError, match="smooth"):
        air.track(frames, smooth=dict(speed=1))


# ---- 4. figure, logger and script -------------------------------------------------------------------------------------------------------
def test_make_trajectory_fig(gpu_device, tmp_path):
    import os
    pytest.importorskip("matplotlib")
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    from attend_infer_repeat_amd.evaluation import make_trajectory_fig
    air, ts, x, y = _mnist_air(8)
    d = procedural_moving_mnist(2, 3, n_objects=(1, 2), seed=5, n_templates=32)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    pred, out = air.predict_frames(frames, 2, birth_score=0.0)
    fig = make_trajectory_fig(frames, out, 3, str(tmp_path), 7)
    assert fig is not None and os.path.getsize(os.path.join(tmp_path, "trajectory_fig_7.png")) > 0 and tuple(pred.shape) == (2, 2, 50, 50)


def test_training_script_track_smooth_options(gpu_device, tmp_path, capsys):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5",
                            "--track-smooth", "2e-4,1e-4,4e-4", "--track-predict", "2"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count("smooth_mota") == 2
    for l in rec:
        assert l["rows_observed"] == l["track_matched"] + l["track_born"] and l["rows_filled"] >= 0
        assert l["smooth_misses"] >= 0 and (l["smooth_mota"] <= 1.0 or np.isnan(l["smooth_mota"]))
    sm = air.track_smoother
    assert sm.horizon == 2 and sm.process_noise == (2e-4, 1e-4) and tuple(air.tracked["frames_pred"].shape[:2]) == (16, 2)
    for bad in (["--track-smooth"], ["--track-eval", "4", "--track-smooth", "1,2"], ["--track-eval", "4", "--track-smooth", "0,1,1"],
                ["--track-eval", "4", "--track-predict", "17"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(bad)
