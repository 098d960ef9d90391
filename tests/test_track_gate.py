"""GPU tests of the Mahalanobis gate of motion-predicted association (air_track_associate_motion_gated, csrc/track_kernels.hip;
track.SequenceTracker(motion=, motion_gate=)): the entry through ctypes against track.reference_associate_motion(gate=) bit for bit on
rows whose decisions are not within rounding of flipping (every d2 at least MARGIN from the gate, every greedy round decided by at
least MARGIN -- track_motion_cases.random_case redraws until they are), the scenarios end to end, the argument checks, the entry
without the gate undisturbed, and the tracker, the model and the training script with the gate.

Bars.  Everything is compared by bits: the integers, `affinity` (the float64 aff rounded once), pred_where / pred_boxes as without the
gate, and pred_d2 (float64: four differences, four products, four IEEE quotients and three sums in one fixed order with contraction
off, rounded once to fp32)."""
import numpy as np
import pytest
import torch

import track_gate_cases as GC
import track_motion_cases as MC
from test_track_motion import DTYPES, check, dev_t, device_idsw, planted_tracker, run_entry, sentinel, shapes_of

from attend_infer_repeat_amd import track, trajectory

pytestmark = pytest.mark.gpu


def run_gated(case, **kw):
    """air_track_associate_motion_gated alone (current stream); every output and a tail behind it start as a sentinel fill.
    case["kw"]: the rule and noise arguments and `gate` (the rest: the defaults); kw overrides single arguments of the call"""
    from attend_infer_repeat_amd import hip as Hh
    T, A, S, F = case["T"], case["A"], case["S"], case["F"]
    R, keys = S * F, GC.GATED_OUTPUTS
    shapes, dtypes = dict(shapes_of(T, S, F), pred_d2=(T, R)), dict(DTYPES, pred_d2=torch.float32)
    bufs = {k: sentinel(shapes[k], dtypes[k]) for k in keys}
    d = {k: dev_t(case[k]) for k in ("what", "where", "boxes", "score")}
    d["n"] = dev_t(case["n"].astype(np.int32))
    p = Hh._p
    rule = dict(track.DEFAULTS, matching="greedy", gate=GC.GATE, **trajectory.DEFAULTS)
    rule.update(case.get("kw", {}))
    a = dict(what=p(d["what"]), where=p(d["where"]), boxes=p(d["boxes"]), score=p(d["score"]), n=p(d["n"]), T=T, S=S, F=F, R=R, A=A,
             H=case["img"][0], W=case["img"][1], q_shift=rule["process_noise"][0], q_scale=rule["process_noise"][1], **rule)
    a["matching"] = track.MATCHINGS.index(a["matching"]) if a["matching"] in track.MATCHINGS else a["matching"]
    a.update({k: p(bufs[k][0]) for k in keys})
    a.update(kw)
    st = Hh.lib().air_track_associate_motion_gated(
        a["what"], a["where"], a["boxes"], a["score"], a["n"], a["T"], a["S"], a["F"], a["R"], a["A"], a["H"], a["W"],
        float(a["iou_gate"]), float(a["appearance_weight"]), float(a["birth_score"]), int(a["max_age"]), int(a["matching"]),
        float(a["q_shift"]), float(a["q_scale"]), float(a["measurement_noise"]), float(a["velocity_var"]), float(a["gate"]),
        *[a[k] for k in keys], Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k in keys:
        n = int(np.prod(shapes[k]))
        got[k] = bufs[k][0][:n].view(shapes[k]).cpu().numpy()
        clean = clean and bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, clean, {k: bufs[k][1] for k in keys}


def within_margins(ref, S):
    return (ref["gate_margin"] >= MC.MARGIN).all() and (ref.get("round_margin", np.full(S, np.inf)) >= MC.MARGIN).all()


# ---- 1. the entry against the reference ------------------------------------------------------------------------------------------------
# the issue's shapes: T = 4, A = 3, S = 2, F = 9, max_age 3; the smallest call; A = 8 and 11 (the unrolled msd loop and its tail); the
# three noise settings -- each with both matchings
ENTRY_PARAMS = [(4, 3, 2, 9, 3, "defaults"), (1, 1, 1, 1, 0, "defaults"), (4, 8, 2, 9, 1, "stiff"), (4, 11, 2, 9, 3, "loose")]


@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("T,A,S,F,max_age,noise", ENTRY_PARAMS)
def test_the_gated_entry_is_the_reference_bit_for_bit(gpu_device, T, A, S, F, max_age, noise, matching):
    kw = dict(iou_gate=0.2, appearance_weight=0.6, birth_score=0.4) if A == 8 else {}
    case, ref = MC.random_case(T, A, S, F, seed=T + A + S + F + max_age, max_age=max_age, matching=matching, noise=MC.NOISE[noise],
                               gate=GC.GATE, **kw)
    st, got, clean, _ = run_gated(case)
    assert st == 0 and clean
    check(got, ref, GC.GATED_OUTPUTS)
    print("states", ref["state_counts"].sum(0).tolist(), "tracks", ref["num_tracks"].tolist())
    assert (got["state_counts"].sum(1) == T * F).all()
    matched = got["obj_state"] == track.MATCHED
    assert not got["pred_d2"][~matched].any() and (got["pred_d2"][matched] <= np.float32(GC.GATE)).all()
    assert F == 1 or matched.sum() >= 4


@pytest.mark.parametrize("gate", [1e-300, 1e300])
@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_a_gate_that_admits_nothing_and_one_that_admits_everything(gpu_device, matching, gate):
    case, ref = MC.random_case(4, 3, 2, 9, seed=2, max_age=3, matching=matching, gate=gate)
    if gate < 1:                                                   # nothing links: every object is born or unconfirmed (or not finite)
        assert not ref["state_counts"][:, [track.MATCHED, track.OVERFLOW]].any() and ref["state_counts"][:, track.BORN].sum() >= 20
    else:                                                          # every live track finds an object while finite ones are left
        assert ref["state_counts"][:, track.MATCHED].sum() >= 20 and ref["pred_d2"].max() > np.float32(GC.GATE)
    st, got, clean, _ = run_gated(case)
    assert st == 0 and clean
    check(got, ref, GC.GATED_OUTPUTS)


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_all_32_slots_predict_and_advance_in_one_frame(gpu_device, matching):
    case = MC.full_table_case(matching=matching)
    case["kw"] = dict(case["kw"], gate=GC.GATE)
    ref = MC.associate_motion(case, return_margins=True, **case["kw"])
    assert within_margins(ref, 1)
    assert ref["state_counts"][0].tolist() == [0, 64, 32, 0, 0, 0] and (ref["track_id"][:, 2] == np.arange(32)).all()
    assert (ref["pred_d2"][:, 1:] > 0).all()
    st, got, clean, _ = run_gated(case)
    assert st == 0 and clean
    check(got, ref, GC.GATED_OUTPUTS)


def test_overflow_with_32_live_tracks(gpu_device):
    case = MC.full_table_case()
    late = MC.rows_from_where([lambda f: (0.1, 0.9, 0.1, 0.9)], 3, 32, A=8)      # a 33rd object, far from the grid, in frames 1 and 2
    for f in (1, 2):
        case["where"][:, f] = np.roll(case["where"][:, f], 1, 0)
        case["what"][:, f], case["score"][:, f] = np.roll(case["what"][:, f], 1, 0), 0.9
        case["where"][0, f] = late["where"][0, f]
    case["boxes"] = MC.scene_boxes(case["where"], MC.IMG).astype(np.float32)
    case["kw"] = dict(case["kw"], gate=GC.GATE)
    ref = MC.associate_motion(case, return_margins=True, **case["kw"])
    assert within_margins(ref, 1) and ref["state_counts"][0, track.OVERFLOW] >= 1 and ref["state_counts"][0, track.BORN] == 32
    assert ref["obj_state"][0, 2] == track.OVERFLOW                # the sequence ENDS in an overflow: the 33rd object of the last frame
    st, got, clean, _ = run_gated(case)
    assert st == 0 and clean
    check(got, ref, GC.GATED_OUTPUTS)


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_planted_nan_inf_and_a_where_row_beyond_every_gate(gpu_device, matching):
    case, _ = MC.random_case(4, 8, 2, 9, seed=3, max_age=2, matching=matching, gate=GC.GATE)
    assert not np.isfinite(case["where"]).all() and not np.isfinite(case["boxes"]).all()      # planted by the case builder
    r0 = int(np.flatnonzero(case["n"][:9] > 1)[0])                 # and in `what`, here: a NaN and an inf in one frame of sequence 0
    case["what"][0, r0, 0], case["what"][1, r0, -1] = np.nan, -np.inf
    # sequence 1: one object whose shift jumps by up to 3e38 a frame.  e^2 is then about 1e77 -- finite in float64, which the fp32
    # rows cannot overflow -- and d2 about 1e80: inadmissible, and float32(d2), which WOULD be inf, is never written
    big = np.float32(3e38)
    rows = slice(9, 18)
    case["n"][rows] = 1
    case["n"][[9 + 3, 9 + 4]] = 0
    case["where"][0, rows] = [[0.2, tx, 0.2, 0.0] for tx in big * np.array([-1, -0.5, 0.5, 1, 1, 1, 1, 1, 1], np.float32)]
    case["boxes"][0, rows], case["score"][0, rows], case["what"][0, rows] = (5.0, 5.0, 10.0, 10.0), 0.9, 0.0
    ref = MC.associate_motion(case, return_margins=True, **case["kw"])
    assert within_margins(ref, 2) and (ref["state_counts"][:, track.NONFINITE] > 0).any()
    jump = ref["obj_state"][0, 9:12]
    assert jump.tolist() == [track.BORN] * 3                       # the boxes coincide (IoU 1): only the gate keeps them apart
    assert (ref["obj_state"][0, 15:18] == track.MATCHED).all() and not ref["pred_d2"][0, 15:18].any()      # at rest: d2 = 0
    assert (ref["obj_state"][:2, r0] == track.NONFINITE).all()
    for k in ("pred_d2", "affinity", "pred_boxes"):
        assert np.isfinite(ref[k]).all(), k
    st, got, clean, _ = run_gated(case)
    assert st == 0 and clean
    check(got, ref, GC.GATED_OUTPUTS)


# ---- 2. the scenarios end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("name", sorted(GC.SCENARIOS))
def test_the_scenarios_on_the_device(gpu_device, name, matching):
    spec = GC.SCENARIOS[name]
    case = MC.scenario(spec, S=2)
    case["kw"] = dict(MC.KW, max_age=spec["max_age"], matching=matching, gate=GC.GATE)
    st, got, clean, _ = run_gated(case)
    assert st == 0 and clean and MC.frame_ids(case, got) == spec["ids"]
    check(got, MC.associate_motion(case, **case["kw"]), GC.GATED_OUTPUTS)
    if name != "CLUTTER":                                          # (B is a second object there: a new id is right)
        assert device_idsw(case, got["track_id"]) == 0
    # the entry without the gate on the same rows: its own reference, and the ids the gate changes (or does not)
    plain = dict(case, kw={k: v for k, v in case["kw"].items() if k != "gate"})
    st, motion, clean, _ = run_entry(plain)
    assert st == 0 and clean and MC.frame_ids(case, motion) == spec["ids_iou_gate"]
    check(motion, MC.associate_motion(plain, **plain["kw"]))


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_the_entry_without_the_gate_is_undisturbed(gpu_device, matching):
    """air_track_associate_motion on the rows of the gated comparison equals its own reference, before and after a gated launch"""
    case, _ = MC.random_case(4, 3, 2, 9, seed=2, max_age=3, matching=matching, gate=GC.GATE)
    plain = dict(case, kw={k: v for k, v in case["kw"].items() if k != "gate"})
    ref = MC.associate_motion(plain, return_margins=True, **plain["kw"])
    st, before, clean, _ = run_entry(plain)
    assert st == 0 and clean
    assert run_gated(case)[0] == 0
    st, after, clean, _ = run_entry(plain)
    assert st == 0 and clean
    check(after, before)
    if within_margins(ref, 2):                                     # (the rows were drawn for the margins of the GATED rule)
        check(after, ref)
    else:
        print("the rule without the gate is within rounding of a flip on these rows: compared before / after only")


# ---- 3. argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case, _ = MC.random_case(4, 3, 2, 5, seed=8, gate=GC.GATE)
    off = torch.zeros(4 * 10 * 4 + 1, device="cuda")
    nan, inf = float("nan"), float("inf")
    for kw, code in ((dict(gate=0.0), -2), (dict(gate=-1.0), -2), (dict(gate=nan), -2), (dict(gate=inf), -2), (dict(gate=-inf), -2),
                     (dict(pred_d2=None), -1), (dict(what=None), -1), (dict(where=None), -1), (dict(pred_where=None), -1),
                     (dict(pred_boxes=None), -1), (dict(track_id=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(R=9), -2),
                     (dict(H=0), -2), (dict(matching=2), -2), (dict(iou_gate=1.0), -2), (dict(max_age=-1), -2), (dict(q_shift=0.0), -2),
                     (dict(measurement_noise=1e-150), -2), (dict(velocity_var=1e4), -2), (dict(where=Hh._p(off[1:])), -3),
                     (dict(boxes=Hh._p(off[1:])), -3), (dict(pred_where=Hh._p(off[1:])), -3), (dict(pred_boxes=Hh._p(off[2:])), -3)):
        st, got, clean, fill = run_gated(case, **kw)
        assert st == code, kw
        assert clean and all((got[k] == fill[k]).all() for k in got), kw
    odd = torch.zeros(4 * 10 + 1, dtype=torch.uint8, device="cuda")      # pred_d2: 4-byte aligned
    st, got, clean, fill = run_gated(case, pred_d2=Hh._p(odd[1:]))
    assert st == -3 and clean and all((got[k] == fill[k]).all() for k in got)


# ---- 4. SequenceTracker(motion=, motion_gate=) on planted provider rows ---------------------------------------------------------------------
def test_the_tracker_with_the_gate_on_planted_rows(gpu_device):
    from test_parse import e2e_case
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    ocfg, spec = e2e_case("tiny")[0], GC.CLUTTER
    T, A, img = ocfg.max_steps, ocfg.n_appearance, tuple(ocfg.img_size)
    S, F = 2, spec["F"]
    case = MC.rows_from_where(spec["objects"], F, T, A=A, S=S, img=img)
    kw = dict(MC.KW, max_age=spec["max_age"], motion=True, motion_gate=True)
    _, _, eager, _ = planted_tracker(case, **kw)
    _, ps, graph, box = planted_tracker(case, capture=True, **kw)
    assert graph._graph is not None and eager._graph is None and graph.motion_gate == track.MOTION_GATE_DEFAULT == eager.motion_gate
    assert graph.launch_count() == {"parser": ps.launch_count(), "track_associate": 1, "track_owner": 1}      # unchanged: one graph, two launches
    assert [e[2] for e in graph._plan] == ["air_track_associate_motion_gated", "air_track_owner"]
    frames = torch.zeros(S, F, *img).cuda()
    ref = MC.associate_motion(case, max_age=spec["max_age"], gate=True, **MC.KW)
    a, b = eager.track(frames), graph.track(frames)
    eager.synchronize(); graph.synchronize()
    keys = GC.GATED_OUTPUTS + ("track_owner",)
    assert set(keys) <= set(b)
    for k in keys:
        assert torch.equal(a[k].view(torch.uint8) if a[k].is_floating_point() else a[k],
                           b[k].view(torch.uint8) if b[k].is_floating_point() else b[k]), k
    check({k: b[k].cpu().numpy() for k in GC.GATED_OUTPUTS}, ref, GC.GATED_OUTPUTS)
    assert MC.frame_ids(case, {"track_id": b["track_id"].cpu().numpy()}) == spec["ids"]
    first = {k: b[k].clone() for k in keys}
    box["case"] = MC.rows_from_where(GC.FAST["objects"], F, T, A=A, S=S, img=img)      # a second call overwrites ...
    c = graph.track(frames)
    graph.synchronize()
    check({k: c[k].cpu().numpy() for k in GC.GATED_OUTPUTS},
          MC.associate_motion(box["case"], max_age=spec["max_age"], gate=True, **MC.KW), GC.GATED_OUTPUTS)
    box["case"] = case                                             # ... and the first rows again give the first bits
    d = graph.track(frames)
    graph.synchronize()
    assert all(torch.equal(d[k].view(torch.uint8) if d[k].is_floating_point() else d[k],
                           first[k].view(torch.uint8) if first[k].is_floating_point() else first[k]) for k in keys)
    # a TrajectorySmoother bound to it runs: A's track with its two frames coasted at the end, and B's single sighting
    sm = TrajectorySmoother(graph)
    sm.capture()
    out = sm.track(frames)
    sm.synchronize()
    assert (out["num_tracks"].cpu().numpy() == 2).all() and "pred_d2" in out
    ids = out["sm_id"].cpu().numpy()
    assert set(np.unique(ids[ids >= 0]).tolist()) == {0, 1}
    # the same rows without the gate: one track, B swallowed
    _, _, plain, _ = planted_tracker(case, **dict(kw, motion_gate=None))
    e = plain.track(frames)
    plain.synchronize()
    assert (e["num_tracks"].cpu().numpy() == 1).all() and "pred_d2" not in e and plain.motion_gate is None
    sm.release_graphs(); graph.release_graphs()


def test_the_tracker_refuses_what_the_entry_refuses(gpu_device):
    from test_parse import e2e_case, make_parser
    from attend_infer_repeat_amd.track import SequenceTracker, StreamTracker
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 8, params)
    with pytest.raises(ValueError, match="needs motion"):
        SequenceTracker(ps, 4, motion_gate=True)
    with pytest.raises(ValueError, match="motion_gate"):
        SequenceTracker(ps, 4, motion=True, motion_gate=float("inf"))
    with pytest.raises(ValueError, match="motion.*stream"):
        StreamTracker(ps, 4, motion_gate=True)


# ---- 5. the model's surface and the training script ----------------------------------------------------------------------------------------
def test_the_gate_on_the_model(gpu_device):
    """AIRonMNIST.track / score_track / tracker / noise_fitter take motion_gate=; the tracker cache keys on it; a stream refuses it;
    the calls without it compute, before and after, what they did"""
    from test_parse import _mnist_air
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    S, F, T = 2, 4, 3
    air, ts, _, _ = _mnist_air(8)
    ts()
    d = procedural_moving_mnist(S, F, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    as_bits = lambda out, keys: {k: (out[k].view(torch.uint8) if out[k].is_floating_point() else out[k]).clone() for k in keys}
    plain, motion = as_bits(air.track(frames), MC.OUTPUTS), as_bits(air.track(frames, motion=True), MC.MOTION_OUTPUTS)
    assert air.tracker(S, F, motion=True, motion_gate=None) is air.tracker(S, F, motion=True) and len(air._trackers) == 2
    out = air.track(frames, motion=True, motion_gate=True)
    tk = air.tracker(S, F, motion=True, motion_gate=True)
    assert tk is not air.tracker(S, F, motion=True) and tk._graph is not None      # a tracker of its own (the cache holds MAX_TRACKERS)
    assert tk.motion_gate == track.MOTION_GATE_DEFAULT and tk is air.tracker(S, F, motion=True, motion_gate=13.2767)
    assert tuple(out["pred_d2"].shape) == (T, S * F) and out["pred_d2"].dtype == torch.float32
    rows = dict(what=out["what"].cpu().numpy().reshape(T, S * F, -1), where=out["where"].cpu().numpy().reshape(T, S * F, 4),
                boxes=out["boxes"].cpu().numpy(), score=out["score"].cpu().numpy(), n=out["num_objects"].cpu().numpy(), F=F, img=(50, 50))
    ref = MC.associate_motion(rows, return_margins=True, gate=True)
    if (ref["gate_margin"] >= MC.MARGIN).all() and (ref["round_margin"] >= MC.MARGIN).all():
        check({k: out[k].cpu().numpy() for k in GC.GATED_OUTPUTS}, ref, GC.GATED_OUTPUTS)
    scores, scored = air.score_track(frames, d["boxes"], accumulate=False, motion=True, motion_gate=True)
    assert scored is tk and tuple(scores["seq_counts"].shape) == (S, 8)
    fit = air.fit_track_noise(frames, motion=True, motion_gate=9.0, birth_score=0.0, fit=False)
    assert fit is None and air.noise_fitter(S, F, motion=True, motion_gate=9.0, birth_score=0.0).tracker.motion_gate == 9.0
    with pytest.raises(ValueError, match="needs motion"):
        air.track(frames, motion_gate=True)
    with pytest.raises(ValueError, match="motion.*stream"):
        air.stream_tracker(S, F, motion_gate=True)
    with pytest.raises(ValueError, match="motion.*stream"):
        air.track_stream(frames, motion_gate=5.0)
    again, again_motion = as_bits(air.track(frames), MC.OUTPUTS), as_bits(air.track(frames, motion=True), MC.MOTION_OUTPUTS)
    assert all(torch.equal(plain[k], again[k]) for k in MC.OUTPUTS)
    assert all(torch.equal(motion[k], again_motion[k]) for k in MC.MOTION_OUTPUTS)


def test_training_script_track_motion_gate_option(gpu_device, tmp_path):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "1", "--log-every", "1000", "--save-every", "1000", "--synthetic-samples", "256", "--eval-batches", "1",
                            "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "4:2.5", "--track-motion",
                            "--track-motion-gate", "--track-fit-noise"])
    air._engine.synchronize()
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0] and all(l["motion_gate"] == track.MOTION_GATE_DEFAULT and "motion" in l for l in rec)
    fits = [l for l in lines if l["data"] == "test_track_noise_fit"]
    assert len(fits) == 1
    for tag in ("defaults", "fit"):                                # under the gate, beside every fit that was not refused
        under = [l for l in lines if l["data"] == "test_motion_%s_track_score" % tag]
        assert len(under) == len([l for l in fits if "refused" not in l]) and all(l["motion_gate"] == track.MOTION_GATE_DEFAULT for l in under)
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-motion-gate"])      # goes with --track-motion
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-motion", "--track-motion-gate", "0"])
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-motion", "--track-motion-gate", "wide"])
