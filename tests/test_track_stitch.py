"""GPU tests of stitching (air_track_stitch, csrc/track_kernels.hip; track.TrackStitcher; AIRonMNIST.track(stitch=)): the entry through
ctypes against track.reference_stitch bit for bit on every output -- the planted scenarios, the seeded random batches (planted NaN /
inf included), the 32-track and the 33-track case, gates that admit nothing and everything --, the argument checks, the stage on
planted provider rows (eager against graph replay, run to run, what it only reads, its owner map, its metrics), and the model and the
training script with stitch=.

Bars.  Everything is compared by bits.  The floats a decision rests on are float64 from the statements of the tracker's own filter
(+ - * / with contraction off, in one order), the solver is int64: there is no tolerance to state.  stitch_d2 and stitch_affinity are
those float64 values rounded once to fp32."""
import numpy as np
import pytest
import torch

import track_motion_cases as MC
import track_stitch_cases as SC
from test_track_motion import bits, dev_t, planted_tracker, sentinel

from attend_infer_repeat_amd import track, trajectory

pytestmark = pytest.mark.gpu

FLOATS = ("stitch_d2", "stitch_affinity")
INPUTS = ("track_id", "num_tracks") + SC.TABLES


def shapes_of(T, S, F):
    per_track, tables = {k: (S, 32) for k in track.STITCH_PER_TRACK}, {k: (S, F * T) for k in track.STITCH_TABLES}
    return dict(per_track, stitch_id=(T, S * F), num_links=(S,), stitch_status=(S,), **tables)


def run_stitch(case, tracks, stitch=None, **kw):
    """air_track_stitch alone (current stream) on the rows of a case and a tracker's output; every output and a tail behind it start
    as a sentinel fill.  stitch: the rule and noise arguments (the rest: the defaults); kw overrides single arguments of the call"""
    from attend_infer_repeat_amd import hip as Hh
    T, A, S, F = case["what"].shape[0], case["what"].shape[2], case["what"].shape[1] // case["F"], case["F"]
    keys, shapes = track.STITCH_OUTPUTS, shapes_of(T, S, F)
    bufs = {k: sentinel(shapes[k], torch.float32 if k in FLOATS else torch.int32) for k in keys}
    d = {k: dev_t(case[k]) for k in ("what", "where")}
    d.update({k: dev_t(np.asarray(tracks[k]).astype(np.int32)) for k in INPUTS})
    p = Hh._p
    rule = dict(max_gap=track.STITCH_MAX_GAP, gate_d2=track.MOTION_GATE_DEFAULT, appearance_weight=track.DEFAULTS["appearance_weight"],
                **trajectory.DEFAULTS)
    given = dict(stitch or {})
    if "gate" in given:
        given["gate_d2"] = track.MOTION_GATE_DEFAULT if given["gate"] is True else given["gate"]
        del given["gate"]
    rule.update(given)
    a = dict({k: p(v) for k, v in d.items()}, T=T, S=S, F=F, R=S * F, A=A, q_shift=rule["process_noise"][0],
             q_scale=rule["process_noise"][1], **rule)
    a.update({k: p(bufs[k][0]) for k in keys})
    a.update(kw)
    values = [a[n] for n in track.STITCH_ARGS]
    at = track.STITCH_ARGS.index("gate_d2")
    values[at:at + 6] = [float(v) for v in values[at:at + 6]]
    st = Hh.lib().air_track_stitch(*values, Hh._stream())
    torch.cuda.synchronize()
    got, clean = {}, True
    for k in keys:
        n = int(np.prod(shapes[k]))
        got[k] = bufs[k][0][:n].view(shapes[k]).cpu().numpy()
        clean = clean and bool((bufs[k][0][n:] == bufs[k][1]).all())
    return st, got, clean, {k: bufs[k][1] for k in keys}


def check(got, ref, what=""):
    for k in track.STITCH_OUTPUTS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(bits(got[k]), bits(ref[k])), (what, k, got[k], ref[k])


# ---- 1. the entry against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [None, {}], ids=["last_box", "motion"])
@pytest.mark.parametrize("name", sorted(SC.SCENARIOS))
def test_the_scenarios_on_the_device(gpu_device, name, motion):
    spec = SC.SCENARIOS[name]
    case = SC.scenario(spec, S=2)
    out = SC.tracked(case, motion)
    ref = SC.stitch(case, out, **spec.get("stitch", {}))
    st, got, clean, _ = run_stitch(case, out, spec.get("stitch"))
    assert st == 0 and clean
    check(got, ref, name)
    assert got["stitch_parent"][0, :len(spec["parent"])].tolist() == spec["parent"] and got["num_links"].tolist() == [spec["links"]] * 2


@pytest.mark.parametrize("gate", [True, 1e-300, 1e300])
@pytest.mark.parametrize("T,A,S,F,seed,max_age,motion", SC.RANDOM)
def test_the_random_batches_bit_for_bit(gpu_device, T, A, S, F, seed, max_age, motion, gate):
    """tests/test_track_stitch_host.py asserts that these batches link, refuse by the gate and by max_gap, and hold non-finite rows"""
    case, tracks = SC.random_case(T, A, S, F, seed, max_age, motion)
    rule = dict(SC.RANDOM_STITCH, gate=gate)
    ref = SC.stitch(case, tracks, **rule)
    st, got, clean, _ = run_stitch(case, tracks, rule)
    assert st == 0 and clean
    check(got, ref)
    if gate == 1e-300:                                             # exact consequence 1: the tracker's bits
        assert not got["num_links"].any() and np.array_equal(got["stitch_id"], tracks["track_id"])
        assert all(np.array_equal(got["stitch_" + k[6:]], tracks[k]) for k in SC.TABLES)
    elif gate == 1e300:
        assert got["num_links"].sum() >= ref["num_links"].sum() > 0 and np.isfinite(got["stitch_d2"]).all()
    print("links", got["num_links"].tolist())


@pytest.mark.parametrize("noise", ["stiff", "loose"])
def test_the_corners_of_the_noise_domain(gpu_device, noise):
    terms = MC.NOISE[noise]
    for name in ("CHAIN", "TWO_BEHIND"):
        case = SC.scenario(SC.SCENARIOS[name], S=2)
        out = SC.tracked(case)
        st, got, clean, _ = run_stitch(case, out, terms)
        assert st == 0 and clean
        check(got, SC.stitch(case, out, **terms), name)


def test_full_32_tracks_and_overflow_at_33(gpu_device):
    for n_before, status, links in ((16, 0, 16), (17, 1, 0)):
        case = SC.full_case(n_before, 16)
        out = SC.tracked(case, appearance_weight=0.25)
        ref = SC.stitch(case, out)
        assert out["num_tracks"][0] == n_before + 16 and ref["stitch_status"][0] == status and ref["num_links"][0] == links
        st, got, clean, _ = run_stitch(case, out)
        assert st == 0 and clean
        check(got, ref, "%d tracks" % (n_before + 16))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_inconsistent_tables_stay_in_bounds_and_equal_the_reference(gpu_device, seed):
    """first / last frames outside the sequence, num_tracks below 0, above F T and above 32, ids beyond N and twice in a frame: the
    kernel clips as the rule says, writes nothing past its outputs (the sentinel tails) and gives the reference's bits"""
    case, tracks = SC.inconsistent_case(seed)
    rule = dict(max_gap=4, gate=1e300)
    st, got, clean, _ = run_stitch(case, tracks, rule)
    assert st == 0 and clean
    check(got, SC.stitch(case, tracks, **rule))


def test_two_launches_give_the_same_bits(gpu_device):
    case, tracks = SC.random_case(*SC.RANDOM[0])
    a, b = run_stitch(case, tracks, SC.RANDOM_STITCH)[1], run_stitch(case, tracks, SC.RANDOM_STITCH)[1]
    check(a, b)


# ---- 2. argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = SC.scenario(SC.LONG_OCCLUSION, S=2)
    out = SC.tracked(case)
    off = torch.zeros(4 * 24 + 1, device="cuda")
    odd = torch.zeros(4 * 64 + 1, dtype=torch.uint8, device="cuda")
    nan, inf = float("nan"), float("inf")
    for kw, code in ((dict(what=None), -1), (dict(where=None), -1), (dict(track_id=None), -1), (dict(num_tracks=None), -1),
                     (dict(track_gaps=None), -1), (dict(stitch_id=None), -1), (dict(stitch_d2=None), -1), (dict(stitch_status=None), -1),
                     (dict(T=0), -2), (dict(T=33), -2), (dict(R=9), -2), (dict(S=0), -2), (dict(A=0), -2), (dict(T=32, F=1024), -2),
                     (dict(max_gap=0), -2), (dict(max_gap=-3), -2), (dict(gate_d2=0.0), -2), (dict(gate_d2=-1.0), -2),
                     (dict(gate_d2=nan), -2), (dict(gate_d2=inf), -2), (dict(appearance_weight=-0.1), -2),
                     (dict(appearance_weight=1.5), -2), (dict(appearance_weight=nan), -2), (dict(q_shift=0.0), -2),
                     (dict(measurement_noise=1e-150), -2), (dict(velocity_var=1e4), -2), (dict(where=Hh._p(off[1:])), -3),
                     (dict(what=Hh._p(odd[1:])), -3), (dict(stitch_root=Hh._p(odd[1:])), -3), (dict(num_links=Hh._p(odd[2:])), -3)):
        st, got, clean, fill = run_stitch(case, out, **kw)
        assert st == code, kw
        assert clean and all((got[k] == fill[k]).all() for k in got), kw


# ---- 3. TrackStitcher on planted provider rows ------------------------------------------------------------------------------------------------
def as_bits(t):
    return t.view(torch.uint8) if t.is_floating_point() else t


@pytest.mark.parametrize("motion", [None, True], ids=["last_box", "motion"])
def test_the_stitcher_on_planted_rows(gpu_device, motion):
    from test_parse import e2e_case
    from attend_infer_repeat_amd import hip as Hh
    from attend_infer_repeat_amd.track import TrackStitcher
    ocfg, spec = e2e_case("tiny")[0], SC.TWO_BEHIND
    T, A, img = ocfg.max_steps, ocfg.n_appearance, tuple(ocfg.img_size)
    S, F = 2, spec["F"]
    case = MC.rows_from_where(spec["objects"], F, T, A=A, S=S, img=img)
    kw = dict(MC.KW, max_age=spec["max_age"], motion=motion, matching="optimal" if motion else "greedy")
    _, _, tk_eager, _ = planted_tracker(case, **kw)
    _, ps, tk, box = planted_tracker(case, capture=True, **kw)
    eager, graph = TrackStitcher(tk_eager), TrackStitcher(tk)
    graph.capture()
    assert graph._graph is not None and eager._graph is None
    assert graph.launch_count() == {"tracker": tk.launch_count(), "track_stitch": 1, "track_owner": 1}
    assert [e[2] for e in graph._plan] == ["air_track_stitch", "air_track_owner"]
    assert graph.max_gap == 8 and graph.gate == track.MOTION_GATE_DEFAULT and graph.appearance_weight == tk.appearance_weight == 0.0
    assert graph.noise == (tk.motion if motion else track.check_motion(True))
    frames = torch.zeros(S, F, *img).cuda()
    a, b = eager.stitch(frames), graph.stitch(frames)
    eager.synchronize(); graph.synchronize()
    keys = track.STITCH_OUTPUTS + ("stitch_owner",)
    assert set(keys) <= set(b) and b["track_id"] is tk.track_id and b["track_owner"] is tk.track_owner      # the tracker's dict, untouched
    for k in keys:
        assert torch.equal(as_bits(a[k]), as_bits(b[k])), k
    host = lambda out, ks: {k: out[k].cpu().numpy() for k in ks}
    tracks = host(b, INPUTS)
    ref = SC.stitch(case, tracks, appearance_weight=0.0)
    check(host(b, track.STITCH_OUTPUTS), ref)
    n = len(spec["parent"])
    assert ref["stitch_parent"][0, :n].tolist() == spec["parent"] and ref["num_links"].tolist() == [2, 2]
    # its owner map: air_track_owner applied to stitch_id
    want = torch.full_like(graph.track_owner, 77)
    assert Hh.lib().air_track_owner(Hh._p(ps.owner), Hh._p(graph.stitch_id), T, S * F, img[0], img[1], Hh._p(want), Hh._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(want, graph.track_owner) and b["stitch_owner"] is graph.track_owner and graph.track_owner is not tk.track_owner
    # what it only reads: the tracker's and the provider's buffers are the bits they were
    read = dict(what=tk._rows["what"], where=tk._rows["where"], boxes=ps.boxes, score=ps.score, num_objects=ps.num_objects, owner=ps.owner,
                track_owner=tk.track_owner, obj_state=tk.obj_state, affinity=tk.affinity, **{k: getattr(tk, k) for k in INPUTS})
    before = {k: v.clone() for k, v in read.items()}
    first = {k: b[k].clone() for k in keys}
    c = graph.run()                                                # a second run on the same tracks: the same bits, nothing else moved
    graph.synchronize()
    assert all(torch.equal(as_bits(c[k]), as_bits(first[k])) for k in keys)
    assert all(torch.equal(as_bits(v), as_bits(before[k])) for k, v in read.items())
    # the metrics on the stitched ids
    gt = case["gt"]
    scored = graph.score(gt, identity=True, accumulate=False)
    hota = graph.hota(gt, accumulate=False)
    graph.synchronize()
    ids = b["stitch_id"].cpu().numpy()
    rs, ri = track.reference_score(case["boxes"], case["n"], ids, gt, F), track.reference_identity(case["boxes"], case["n"], ids, gt, F)
    rh = track.reference_hota(case["boxes"], case["n"], ids, gt, F)
    for k, want_k in (("seq_counts", rs["seq_counts"]), ("seq_iou", rs["seq_iou"]), ("gt_match", rs["gt_match"]), ("seq_idf", ri["seq_idf"]),
                      ("idf_overlap", ri["overlap"])):
        assert np.array_equal(bits(scored[k].cpu().numpy()), bits(want_k)), k
    for k in ("seq_hota_i", "seq_hota_f", "hota_potential", "hota_id_count", "hota_gt_count", "hota_matches"):
        assert np.array_equal(bits(hota[k].cpu().numpy()), bits(rh[k])), k
    assert graph.identity_summary()["idf1"] == 1.0 and graph.hota_summary()["assa"] == 1.0 and graph.summary()["id_switches"] == 0
    tk.score(gt, identity=True, accumulate=False)                  # the tracker's own ids on the same rows: split tracks
    assert tk.identity_summary()["idf1"] < 1.0 and graph.identity_summary()["idf1"] == 1.0      # (totals of their own)
    graph.reset()
    assert graph.summary()["gt"] == 0
    # other rows through the same graph, then the first rows again
    box["case"] = MC.rows_from_where(SC.CHAIN["objects"], F, T, A=A, S=S, img=img)
    d = graph.stitch(frames)
    graph.synchronize()
    check(host(d, track.STITCH_OUTPUTS), SC.stitch(box["case"], host(d, INPUTS), appearance_weight=0.0))
    box["case"] = case
    e = graph.stitch(frames)
    graph.synchronize()
    assert all(torch.equal(as_bits(e[k]), as_bits(first[k])) for k in keys)
    graph.release_graphs(); tk.release_graphs()


def test_the_stitcher_refuses_a_stream_and_bad_arguments(gpu_device):
    from test_parse import e2e_case, make_parser
    from attend_infer_repeat_amd.track import SequenceTracker, StreamTracker, TrackStitcher
    ocfg, _, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 8, params)
    with pytest.raises(ValueError, match="out of scope on a stream"):
        TrackStitcher(StreamTracker(ps, 4))
    tk = SequenceTracker(ps, 4)
    for kw, text in ((dict(max_gap=0), "max_gap"), (dict(gate=float("inf")), "motion_gate"), (dict(appearance_weight=2.0), "appearance_weight"),
                     (dict(noise=dict(measurement_noise=1e-150)), "measurement_noise")):
        with pytest.raises(ValueError, match=text):
            TrackStitcher(tk, **kw)
    st = TrackStitcher(tk, max_gap=3, gate=9.0, appearance_weight=0.5, noise=dict(velocity_var=0.0))
    assert (st.max_gap, st.gate, st.appearance_weight, st.noise["velocity_var"]) == (3, 9.0, 0.5, 0.0)


# ---- 4. the model's surface and the training script --------------------------------------------------------------------------------------------
def test_stitch_on_the_model(gpu_device):
    """AIRonMNIST.track / score_track / stitcher take stitch=; the cache keys on it; smooth= and a stream refuse it; the calls without
    it compute, before and after, what they did, with the same tracker object"""
    from test_parse import _mnist_air
    from attend_infer_repeat_amd.data import procedural_moving_mnist
    S, F, T = 2, 6, 3
    air, ts, _, _ = _mnist_air(8)
    ts()
    d = procedural_moving_mnist(S, F, n_objects=(1, 2), seed=3, n_templates=32, return_annotations=True)
    frames = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    snap = lambda out, keys: {k: as_bits(out[k]).clone() for k in keys}
    rule = dict(max_age=0, birth_score=0.0)                        # an untrained model: short tracks, many of them
    plain = snap(air.track(frames, **rule), MC.OUTPUTS)
    tk = air.tracker(S, F, **rule)
    assert air.tracker(S, F, stitch=None, **rule) is tk and len(air._trackers) == 1
    out = air.track(frames, stitch=dict(max_gap=3, gate=1e300), **rule)
    st = air.stitcher(S, F, stitch=dict(max_gap=3, gate=1e300), **rule)
    assert st.tracker is not tk and st.tracker is air.tracker(S, F, stitch=dict(max_gap=3, gate=1e300), **rule) and st._graph is not None
    assert st is air.stitcher(S, F, stitch=dict(max_gap=3, gate=1e300, appearance_weight=None), **rule) and len(air._trackers) == 2
    assert (st.max_gap, st.gate, st.appearance_weight) == (3, 1e300, track.DEFAULTS["appearance_weight"])
    assert tuple(out["stitch_id"].shape) == (T, S * F) and out["stitch_owner"].dtype == torch.int16
    host = lambda ks: {k: out[k].cpu().numpy() for k in ks}
    rows = dict(what=out["what"].cpu().numpy().reshape(T, S * F, -1), where=out["where"].cpu().numpy().reshape(T, S * F, 4), F=F)
    ref = SC.stitch(rows, host(INPUTS), max_gap=3, gate=1e300, return_margins=True)
    print("tracks", out["num_tracks"].tolist(), "links", ref["num_links"].tolist(), "gate margin", ref["gate_margin"].tolist())
    check(host(track.STITCH_OUTPUTS), ref)
    scores, scored = air.score_track(frames, d["boxes"], accumulate=False, identity=True, hota=True, stitch=dict(max_gap=3, gate=1e300), **rule)
    assert scored is st and tuple(scores["seq_counts"].shape) == (S, 8) and "seq_idf" in scores and "seq_hota_i" in scores["hota"]
    ids = air.tracked["stitch_id"].cpu().numpy()
    ri = track.reference_identity(air.tracked["boxes"].cpu().numpy(), air.tracked["num_objects"].cpu().numpy(), ids,
                                  np.asarray(d["boxes"], np.float32), F)
    assert np.array_equal(scores["seq_idf"].cpu().numpy(), ri["seq_idf"])
    with pytest.raises(ValueError, match="stitch= together with smooth="):
        air.track(frames, stitch=True, smooth=True)
    with pytest.raises(TypeError, match="stitch"):
        air.stream_tracker(S, F, stitch=True)
    with pytest.raises(TypeError, match="stitch"):
        air.track_stream(frames, stitch=True)
    with pytest.raises(ValueError, match="max_gap"):
        air.track(frames, stitch=0)
    assert "objects_temporal_kept" in air.track(frames, stitch=2, temporal=1, **rule)       # temporal= is a provider: allowed
    again = snap(air.track(frames, **rule), MC.OUTPUTS)
    assert all(torch.equal(plain[k], again[k]) for k in MC.OUTPUTS) and "stitch_id" not in air.tracked


def test_training_script_track_stitch_option(gpu_device, tmp_path):
    import json
    import os
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "1", "--log-every", "1000", "--save-every", "1000", "--synthetic-samples", "256", "--eval-batches", "1",
                            "--summary-every", "0", "--results-dir", str(tmp_path), "--track-eval", "6:2.5", "--track-stitch", "3,20.5",
                            "--track-identity", "--track-hota"])
    air._engine.synchronize()
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_track_score"]
    assert [l["step"] for l in rec] == [0] and rec[0]["stitch"] == dict(max_gap=3, gate=20.5, appearance_weight=track.DEFAULTS["appearance_weight"])
    for k in ("mota", "idf1", "hota", "stitch_mota", "stitch_id_switches", "stitch_links", "stitch_idf1", "stitch_hota", "stitch_assa"):
        assert k in rec[0], k
    for bad in (["--track-stitch"], ["--track-eval", "4", "--track-stitch", "0"], ["--track-eval", "4", "--track-stitch", "wide"],
                ["--track-eval", "4", "--track-stitch", "3,0"], ["--track-eval", "4", "--track-stitch", "3,4,5"],
                ["--track-eval", "4", "--track-stitch", "--track-stream", "2"], ["--track-eval", "4", "--track-stitch", "--track-smooth"],
                ["--track-eval", "4", "--track-stitch", "--track-predict", "2"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(bad)
