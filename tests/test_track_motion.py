"""GPU tests of motion-predicted association (air_track_associate_motion, csrc/track_kernels.hip; track.SequenceTracker(motion=)):
the entry through ctypes against track.reference_associate_motion bit for bit on rows whose decisions are not within rounding of
flipping (every IoU at least MARGIN from the gate, every greedy round decided by at least MARGIN -- track_motion_cases.random_case
redraws until they are), the two exact consequences on the device, the scenarios end to end, the unchanged instantiations, the argument
checks, and the tracker with motion on planted provider rows.

Bars.  Everything is compared by bits: the integers, `affinity` (the float64 aff rounded once), and pred_where / pred_boxes (the
float64 state advanced by the statements of trajectory._filter_step in their order with contraction off, one product and one sum for
the prediction, rounded once; the box operation by operation in fp32)."""
import numpy as np
import pytest
import torch

import track_motion_cases as MC
from test_parse import SENTINEL_F, SENTINEL_I, e2e_case, make_parser
from test_track_host import crafted_rows

from attend_infer_repeat_amd import track, trajectory

pytestmark = pytest.mark.gpu

TAIL = 64
dev_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
DTYPES = dict(track_id=torch.int32, obj_state=torch.int8, affinity=torch.float32, prev_frame=torch.int32, prev_slot=torch.int32,
              num_tracks=torch.int32, track_first=torch.int32, track_last=torch.int32, track_length=torch.int32, track_gaps=torch.int32,
              state_counts=torch.int32, pred_where=torch.float32, pred_boxes=torch.float32)


def sentinel(shape, dtype, tail=TAIL):
    fill = SENTINEL_F if dtype.is_floating_point else (99 if dtype in (torch.int8, torch.int16) else SENTINEL_I)
    return torch.full((int(np.prod(shape)) + tail,), fill, dtype=dtype, device="cuda"), fill


def shapes_of(T, S, F):
    R = S * F
    return dict(track_id=(T, R), obj_state=(T, R), affinity=(T, R), prev_frame=(T, R), prev_slot=(T, R), num_tracks=(S,),
                track_first=(S, F * T), track_last=(S, F * T), track_length=(S, F * T), track_gaps=(S, F * T), state_counts=(S, 6),
                pred_where=(T, R, 4), pred_boxes=(T, R, 4))


def run_entry(case, entry="air_track_associate_motion", **kw):
    """one association entry alone (current stream); every output and a tail behind it start as a sentinel fill.  case["kw"]: the rule
    and noise arguments (the rest: the defaults); kw overrides single arguments of the call"""
    from attend_infer_repeat_amd import hip as Hh
    motion = entry == "air_track_associate_motion"
    T, A, S, F = case["T"], case["A"], case["S"], case["F"]
    R, keys = S * F, MC.MOTION_OUTPUTS if motion else MC.OUTPUTS
    shapes = shapes_of(T, S, F)
    bufs = {k: sentinel(shapes[k], DTYPES[k]) for k in keys}
    d = {k: dev_t(case[k]) for k in ("what", "where", "boxes", "score")}
    d["n"] = dev_t(case["n"].astype(np.int32))
    p = Hh._p
    rule = dict(track.DEFAULTS, matching="greedy", **trajectory.DEFAULTS)
    rule.update(case.get("kw", {}))
    a = dict(what=p(d["what"]), where=p(d["where"]), boxes=p(d["boxes"]), score=p(d["score"]), n=p(d["n"]), T=T, S=S, F=F, R=R, A=A,
             H=case["img"][0], W=case["img"][1], q_shift=rule["process_noise"][0], q_scale=rule["process_noise"][1], **rule)
    a["matching"] = track.MATCHINGS.index(a["matching"]) if a["matching"] in track.MATCHINGS else a["matching"]
    a.update({k: p(bufs[k][0]) for k in keys})
    a.update(kw)
    rows = (a["what"], a["boxes"], a["score"], a["n"])
    gates = (float(a["iou_gate"]), float(a["appearance_weight"]), float(a["birth_score"]), int(a["max_age"]))
    if motion:
        st = Hh.lib().air_track_associate_motion(
            rows[0], a["where"], *rows[1:], a["T"], a["S"], a["F"], a["R"], a["A"], a["H"], a["W"], *gates, int(a["matching"]),
            float(a["q_shift"]), float(a["q_scale"]), float(a["measurement_noise"]), float(a["velocity_var"]),
            *[a[k] for k in keys], Hh._stream())
    else:
        st = getattr(Hh.lib(), entry)(*rows, a["T"], a["S"], a["F"], a["R"], a["A"], *gates, *[a[k] for k in keys], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k in keys:
        n = int(np.prod(shapes[k]))
        got[k] = bufs[k][0][:n].view(shapes[k]).cpu().numpy()
        clean = clean and bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, clean, {k: bufs[k][1] for k in keys}


def check(got, ref, keys=MC.MOTION_OUTPUTS, what=""):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(bits(got[k]), bits(ref[k])), (what, k, got[k], ref[k])


# ---- 1. the entry against the reference ------------------------------------------------------------------------------------------------
# S in {1, 3}, F in {1, 2, 9}, T in {1, 4}, A in {3, 8, 11} (the tail, one 8-block, a block plus tail of the msd loop), max_age in
# {0, 1, 3}, the noise at the defaults and at two corners of the supported domain -- every value with every matching, not every
# combination
ENTRY_PARAMS = [(4, 3, 3, 9, 3, "defaults"), (4, 8, 1, 9, 1, "stiff"), (4, 11, 3, 9, 3, "loose"), (1, 3, 3, 9, 1, "defaults"),
                (4, 8, 3, 2, 0, "loose"), (1, 11, 1, 1, 0, "stiff"), (4, 11, 1, 9, 0, "defaults"), (4, 3, 1, 2, 3, "stiff")]


@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("T,A,S,F,max_age,noise", ENTRY_PARAMS)
def test_the_entry_is_the_reference_bit_for_bit(gpu_device, T, A, S, F, max_age, noise, matching):
    kw = dict(iou_gate=0.2, appearance_weight=0.6, birth_score=0.4) if (T + A + S + F) % 2 else {}
    case, ref = MC.random_case(T, A, S, F, seed=T + A + S + F + max_age, max_age=max_age, matching=matching, noise=MC.NOISE[noise], **kw)
    st, got, clean, _ = run_entry(case)
    assert st == 0 and clean
    check(got, ref)
    print("states", ref["state_counts"].sum(0).tolist(), "tracks", ref["num_tracks"].tolist())
    assert (got["state_counts"].sum(1) == T * F).all()


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_all_32_slots_live_and_matched_in_one_frame(gpu_device, matching):
    case = MC.full_table_case(matching=matching)
    ref = MC.associate_motion(case, return_margins=True, **case["kw"])
    assert (ref["gate_margin"] >= MC.MARGIN).all() and (ref.get("round_margin", np.full(1, np.inf)) >= MC.MARGIN).all()
    assert ref["state_counts"][0].tolist() == [0, 64, 32, 0, 0, 0] and (ref["track_id"][:, 2] == np.arange(32)).all()
    assert np.abs(ref["pred_where"][:, 2] - case["where"][:, 1]).max() > 1e-3      # by frame 2 every track has a rate
    st, got, clean, _ = run_entry(case)
    assert st == 0 and clean
    check(got, ref)


def test_overflow_with_32_live_tracks(gpu_device):
    case = MC.full_table_case()
    late = MC.rows_from_where([lambda f: (0.1, 0.9, 0.1, 0.9)], 3, 32, A=8)      # a 33rd object, far from the grid, in frames 1 and 2
    for f in (1, 2):
        case["where"][:, f] = np.roll(case["where"][:, f], 1, 0)
        case["what"][:, f], case["score"][:, f] = np.roll(case["what"][:, f], 1, 0), 0.9
        case["where"][0, f] = late["where"][0, f]
    case["boxes"] = MC.scene_boxes(case["where"], MC.IMG).astype(np.float32)
    ref = MC.associate_motion(case, **case["kw"])
    assert ref["state_counts"][0].tolist() == [0, 62, 32, 0, 2, 0] and ref["obj_state"][0, 1] == track.OVERFLOW
    st, got, clean, _ = run_entry(case)
    assert st == 0 and clean
    check(got, ref)


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_planted_nan_inf_and_a_prediction_that_leaves_fp32(gpu_device, matching):
    case, _ = MC.random_case(4, 8, 2, 9, seed=3, max_age=2, matching=matching)
    assert not np.isfinite(case["where"]).all() and not np.isfinite(case["boxes"]).all()      # planted by the case builder
    # sequence 1: one object whose shift overflows fp32 when it is extrapolated (the box of the prediction is not finite: the
    # fallback to the last-sighting box), seen again after a gap; the boxes are given, not derived, so that they stay finite
    big = np.float32(3e38)
    F, rows = 9, slice(9, 18)
    case["n"][rows] = 1
    case["n"][[9 + 3, 9 + 4]] = 0
    case["where"][0, rows] = [[0.2, tx, 0.2, 0.0] for tx in big * np.array([-1, -0.5, 0.5, 1, 1, 1, 1, 1, 1], np.float32)]
    case["boxes"][0, rows], case["score"][0, rows], case["what"][0, rows] = (5.0, 5.0, 10.0, 10.0), 0.9, 0.0
    ref = MC.associate_motion(case, return_margins=True, **case["kw"])
    assert (ref["gate_margin"] >= MC.MARGIN).all() and (ref.get("round_margin", np.full(2, np.inf)) >= MC.MARGIN).all()
    matched = ref["obj_state"][0, rows] == track.MATCHED
    assert matched.sum() >= 5 and not np.isfinite(ref["pred_where"][0, rows][matched]).all()
    assert np.isfinite(ref["pred_boxes"]).all() and (ref["state_counts"][:, track.NONFINITE] > 0).any()
    st, got, clean, _ = run_entry(case)
    assert st == 0 and clean
    check(got, ref)


# ---- 2. the scenarios end to end, and exact consequence 1 -----------------------------------------------------------------------------------
def device_idsw(case, ids):
    from attend_infer_repeat_amd import hip as Hh
    S, F, T, G = case["S"], case["F"], case["T"], case["gt"].shape[1]
    counts, iou = torch.zeros((S, 8), dtype=torch.int32, device="cuda"), torch.zeros((S,), dtype=torch.float64, device="cuda")
    gm = torch.zeros((S * F, G), dtype=torch.int32, device="cuda")
    d = [dev_t(case["boxes"]), dev_t(case["n"].astype(np.int32)), dev_t(ids), dev_t(case["gt"])]
    st = Hh.lib().air_track_score(*[Hh._p(t) for t in d], 0.5, T, G, S, F, S * F, Hh._p(counts), Hh._p(iou), Hh._p(gm), Hh._stream())
    torch.cuda.synchronize()
    assert st == 0
    return int(counts[:, track.COUNTS.index("idsw")].sum())


@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("name", ["OCCLUSION", "CROSSING"])
def test_the_scenarios_on_the_device_keep_their_identities(gpu_device, name, matching):
    spec = getattr(MC, name)
    case = MC.scenario(spec, S=2)
    case["kw"] = dict(MC.KW, max_age=spec["max_age"], matching=matching)
    st, got, clean, _ = run_entry(case)
    assert st == 0 and clean and MC.frame_ids(case, got) == spec["ids"]
    check(got, MC.associate_motion(case, **case["kw"]))
    assert device_idsw(case, got["track_id"]) == 0
    entry = "air_track_associate_optimal" if matching == "optimal" else "air_track_associate"
    st, last_box, clean, _ = run_entry(dict(case, kw={k: v for k, v in case["kw"].items() if k != "matching"}), entry)
    assert st == 0 and clean and MC.frame_ids(case, last_box) == spec["ids_last_box"]
    assert device_idsw(case, last_box["track_id"]) >= 2            # (one or two per sequence: the scenario still discriminates)


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_static_tracks_equal_the_entries_without_motion_bit_for_bit(gpu_device, matching):
    entry = "air_track_associate_optimal" if matching == "optimal" else "air_track_associate"
    cases = [MC.random_case(4, 3, 3, 9, seed=s, max_age=2, matching=matching, static=True, bad=False)[0] for s in (0, 1)]
    cases.append(MC.random_case(4, 8, 3, 2, seed=5, max_age=1, matching=matching, bad=False)[0])      # F = 2: rows that move
    for i, case in enumerate(cases):
        st, motion, clean, _ = run_entry(case)
        assert st == 0 and clean
        rule = {k: v for k, v in case["kw"].items() if k in track.DEFAULTS}
        st, plain, clean, _ = run_entry(dict(case, kw=rule), entry)
        assert st == 0 and clean and (motion["obj_state"] == track.MATCHED).sum() >= 3
        check(motion, plain, MC.OUTPUTS, i)


@pytest.mark.parametrize("entry, matching", [("air_track_associate", "greedy"), ("air_track_associate_optimal", "optimal")])
def test_the_existing_instantiations_are_unchanged(gpu_device, entry, matching):
    """a cheap guard that one more template parameter changed nothing: the entries without motion on the same random rows"""
    for seed, (T, A, S, F) in enumerate([(4, 11, 3, 9), (32, 8, 1, 5)]):
        case, ref = crafted_rows(T, A, S, F, seed=seed + 40, margin=MC.MARGIN)
        ref = track.reference_associate(case["what"], case["boxes"], case["score"], case["n"], F, return_margins=True, matching=matching)
        assert (ref["gate_margin"] >= MC.MARGIN).all()
        case.update(where=np.zeros((T, S * F, 4), np.float32), img=MC.IMG)
        st, got, clean, _ = run_entry(case, entry)
        assert st == 0 and clean
        check(got, ref, MC.OUTPUTS, seed)


# ---- 3. argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, _ = MC.random_case(4, 3, 2, 5, seed=8)
    off = torch.zeros(4 * 10 * 4 + 1, device="cuda")
    nan = float("nan")
    for kw, code in ((dict(what=None), -1), (dict(where=None), -1), (dict(boxes=None), -1), (dict(pred_where=None), -1),
                     (dict(pred_boxes=None), -1), (dict(track_id=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(R=9), -2),
                     (dict(H=0), -2), (dict(W=0), -2), (dict(matching=2), -2), (dict(matching=-1), -2), (dict(iou_gate=1.0), -2),
                     (dict(max_age=-1), -2), (dict(q_shift=0.0), -2), (dict(q_scale=nan), -2), (dict(measurement_noise=0.0), -2),
                     (dict(measurement_noise=1e-150), -2), (dict(q_shift=1e-40), -2), (dict(q_scale=1e13), -2),
                     (dict(velocity_var=1e4), -2), (dict(velocity_var=-1.0), -2), (dict(where=Hh._p(off[1:])), -3),
                     (dict(boxes=Hh._p(off[1:])), -3), (dict(pred_where=Hh._p(off[1:])), -3), (dict(pred_boxes=Hh._p(off[2:])), -3)):
        st, got, clean, fill = run_entry(case, **kw)
        assert st == code, kw
        assert clean and all((got[k] == fill[k]).all() for k in got), kw


# ---- 4. SequenceTracker(motion=) on planted provider rows -------------------------------------------------------------------------------------
def plant(provider, case):
    """overwrite the provider's device buffers with the rows of a case (what a parse of such frames would have left)"""
    from attend_infer_repeat_amd.tile import _provider_rows
    rows = _provider_rows(provider)
    torch.cuda.synchronize()
    for buf, k in ((rows["what"], "what"), (rows["where"], "where"), (provider.boxes, "boxes"), (provider.score, "score"),
                   (provider.num_objects, "n")):
        buf.view(-1).copy_(torch.from_numpy(np.ascontiguousarray(case[k])).reshape(-1).to(buf.dtype))
    torch.cuda.synchronize()


def planted_tracker(case, capture=False, **kw):
    """a SceneParser whose parse() leaves the case's rows in its buffers (the model is untrained), and a tracker bound to it"""
    from attend_infer_repeat_amd.track import SequenceTracker
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, case["S"] * case["F"], params)
    inner, box = ps.parse, {"case": case}

    def planted_parse(*args, **kwargs):
        base = inner(*args, **kwargs)
        plant(ps, box["case"])
        return base

    ps.parse = planted_parse
    tk = SequenceTracker(ps, case["F"], **kw)
    if capture:
        ps.capture()
        tk.capture()
    return ocfg, ps, tk, box


def test_the_tracker_with_motion_on_planted_rows(gpu_device):
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    ocfg, spec = e2e_case("tiny")[0], MC.OCCLUSION
    T, A, img = ocfg.max_steps, ocfg.n_appearance, tuple(ocfg.img_size)
    S, F = 2, spec["F"]
    case = MC.rows_from_where(spec["objects"], F, T, A=A, S=S, img=img)
    kw = dict(MC.KW, max_age=spec["max_age"], motion=True)
    _, _, eager, _ = planted_tracker(case, **kw)
    _, ps, graph, box = planted_tracker(case, capture=True, **kw)
    assert graph._graph is not None and eager._graph is None and graph.motion == track.check_motion(True)
    assert graph.launch_count() == {"parser": ps.launch_count(), "track_associate": 1, "track_owner": 1}
    assert list(graph.segments) == ["associate", "owner"] and [e[2] for e in graph._plan] == ["air_track_associate_motion", "air_track_owner"]
    frames = torch.zeros(S, F, *img).cuda()
    ref = MC.associate_motion(case, max_age=spec["max_age"], **MC.KW)
    a, b = eager.track(frames), graph.track(frames)
    eager.synchronize(); graph.synchronize()
    keys = MC.MOTION_OUTPUTS + ("track_owner",)
    assert set(keys) <= set(b)
    for k in keys:
        assert torch.equal(a[k].view(torch.uint8) if a[k].is_floating_point() else a[k],
                           b[k].view(torch.uint8) if b[k].is_floating_point() else b[k]), k
    check({k: b[k].cpu().numpy() for k in MC.MOTION_OUTPUTS}, ref)
    assert MC.frame_ids(case, {"track_id": b["track_id"].cpu().numpy()}) == spec["ids"]
    first = {k: b[k].clone() for k in keys}
    # a second call overwrites: other rows (the crossing, padded to this tracker's frames), then the first rows again
    other = MC.rows_from_where(MC.CROSSING["objects"], F, T, A=A, S=S, img=img)
    box["case"] = other
    c = graph.track(frames)
    graph.synchronize()
    check({k: c[k].cpu().numpy() for k in MC.MOTION_OUTPUTS}, MC.associate_motion(other, max_age=spec["max_age"], **MC.KW))
    box["case"] = case
    d = graph.track(frames)
    graph.synchronize()
    assert all(torch.equal(d[k], first[k]) for k in ("track_id", "obj_state", "prev_frame", "track_last", "track_owner"))
    assert torch.equal(d["pred_where"].view(torch.int32), first["pred_where"].view(torch.int32))
    # a TrajectorySmoother bound to it runs, and its completed table is ONE unbroken track per sequence
    sm = TrajectorySmoother(graph)
    sm.capture()
    out = sm.track(frames)
    sm.synchronize()
    ids, state = out["sm_id"].cpu().numpy(), out["sm_state"].cpu().numpy()
    assert (ids[0] == 0).all() and (out["sm_count"].cpu().numpy() == 1).all()
    assert state[0].reshape(S, F).tolist() == [[trajectory.OBSERVED] * 4 + [trajectory.FILLED] * 2 + [trajectory.OBSERVED] * 2] * S
    assert (out["num_tracks"].cpu().numpy() == 1).all()
    # the same rows without motion: two fragments, which the smoother smooths separately
    _, _, plain, _ = planted_tracker(case, **dict(kw, motion=None))
    e = plain.track(frames)
    plain.synchronize()
    assert (e["num_tracks"].cpu().numpy() == 2).all() and "pred_where" not in e and plain.motion is None
    sm.release_graphs(); graph.release_graphs()


def test_the_tracker_refuses_what_the_entry_refuses(gpu_device):
    from attend_infer_repeat_amd.track import SequenceTracker, StreamTracker
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 8, params)
    with pytest.raises(ValueError, match="V_OVER_R_MAX"):
        SequenceTracker(ps, 4, motion=dict(velocity_var=1e4))
    with pytest.raises(ValueError, match="unknown keys"):
        SequenceTracker(ps, 4, motion=dict(noise=1.0))
    with pytest.raises(ValueError, match="motion.*stream"):
        StreamTracker(ps, 4, motion=True)


# ---- 5. the model's surface and the training script ----------------------------------------------------------------------------------------
def test_motion_on_the_model(gpu_device):
    """AIRonMNIST.track / score_track / fit_track_noise take motion=; the tracker cache keys on it; motion=True with smooth=dict takes
    the smoother's noise terms and an explicit dict wins; a stream refuses it; motion=None is the call without the argument"""
    from test_parse import _mnist_air
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    S, F, T = 2, 4, 3
    air, ts, _, _ = _mnist_air(8)
    ts()
    d = procedural_moving_mnist(S, F, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    plain = air.track(frames)
    assert "pred_where" not in plain and air.track(frames, motion=None) is not None and len(air._trackers) == 1
    assert air.tracker(S, F, motion=None) is air.tracker(S, F) and air.tracker(S, F).motion is None
    plain = {k: plain[k].clone() for k in MC.OUTPUTS}
    out = air.track(frames, motion=True)
    tk = air.tracker(S, F, motion=True)
    assert len(air._trackers) == 2 and tk is not air.tracker(S, F) and tk._graph is not None and tk.motion == track.check_motion(True)
    assert tuple(out["pred_where"].shape) == tuple(out["pred_boxes"].shape) == (T, S * F, 4)
    rows = dict(what=out["what"].cpu().numpy().reshape(T, S * F, -1), where=out["where"].cpu().numpy().reshape(T, S * F, 4),
                boxes=out["boxes"].cpu().numpy(), score=out["score"].cpu().numpy(), n=out["num_objects"].cpu().numpy(), F=F, img=(50, 50))
    ref = MC.associate_motion(rows, return_margins=True)
    if (ref["gate_margin"] >= MC.MARGIN).all() and (ref["round_margin"] >= MC.MARGIN).all():
        check({k: out[k].cpu().numpy() for k in MC.MOTION_OUTPUTS}, ref)
    # the noise terms: the smoother's with motion=True, an explicit dict wins
    terms = dict(process_noise=(2e-4, 1e-4), measurement_noise=5e-4, velocity_var=0.01)
    both = air.track(frames, motion=True, smooth=terms)
    assert air.tracker(S, F, motion=True, smooth=terms).motion == track.check_motion(terms) and "sm_where" in both and "pred_where" in both
    scores, scored = air.score_track(frames, d["boxes"], accumulate=False, motion=True)
    assert scored.motion == track.check_motion(True) and tuple(scores["seq_counts"].shape) == (S, 8)
    fit = air.fit_track_noise(frames, motion=True, birth_score=0.0, fit=False)
    assert fit is None and air.noise_fitter(S, F, motion=True, birth_score=0.0).tracker.motion == track.check_motion(True)
    with pytest.raises(ValueError, match="motion.*stream"):
        air.stream_tracker(S, F, motion=True)
    with pytest.raises(ValueError, match="motion.*stream"):
        air.track_stream(frames, motion=dict(velocity_var=0.0))
    again = air.track(frames)                                      # the call without motion computes what it did
    assert all(torch.equal(plain[k], again[k]) for k in MC.OUTPUTS)


def test_training_script_track_motion_option(gpu_device, tmp_path, capsys):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "1", "--log-every", "1000", "--save-every", "1000", "--synthetic-samples", "256", "--eval-batches", "1",
                            "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5", "--track-motion",
                            "--track-fit-noise"])
    air._engine.synchronize()
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0] and all(l["motion"]["velocity_var"] == trajectory.DEFAULTS["velocity_var"] for l in rec)
    fits = [l for l in lines if l["data"] == "test_track_noise_fit"]
    assert len(fits) == 1
    for tag in ("defaults", "fit"):                                # logged beside every fit that was not refused
        assert len([l for l in lines if l["data"] == "test_motion_%s_track_score" % tag]) == len([l for l in fits if "refused" not in l])
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-motion"])                       # goes with --track-eval
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-motion", "1e-4,1e-4,4e-4,1e4"])      # outside the domain
