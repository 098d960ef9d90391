"""Host tests of stitching (track.reference_stitch, STITCHING in track.py's module text; no GPU): the planted scenarios against
hand-written links, roots and tables, the exact consequences, the filter states against the tracker's own, the identity figures a
stitched track repairs, the refusals, the planted defects of the reference, and the conditions the seeded random batches of the
device test must meet."""
import types

import numpy as np
import pytest

import track_motion_cases as MC
import track_stitch_cases as SC

from attend_infer_repeat_amd import stacks, track, trajectory


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint8) if x.dtype.kind == "f" else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run(name, S=1, motion=None, **kw):
    spec = SC.SCENARIOS[name]
    case = SC.scenario(spec, S=S)
    out = SC.tracked(case, motion)
    return spec, case, out, SC.stitch(case, out, **dict(spec.get("stitch", {}), **kw))


# ---- 1. the scenarios by hand ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [None, {}], ids=["last_box", "motion"])
@pytest.mark.parametrize("name", sorted(SC.SCENARIOS))
def test_the_scenarios_by_hand(name, motion):
    spec, case, out, st = run(name, S=2, motion=motion)
    F, T = spec["F"], spec["T"]
    assert MC.frame_ids(case, out) == spec["tracker_ids"]           # the tracker splits the tracks as the scenario says
    N = len(spec["parent"])
    for s in range(2):
        assert out["num_tracks"][s] == N and st["stitch_status"][s] == track.STITCHED and st["num_links"][s] == spec["links"]
        assert st["stitch_parent"][s].tolist() == spec["parent"] + [-1] * (32 - N)
        assert st["stitch_root"][s].tolist() == spec["root"] + [-1] * (32 - N)
        for k in ("first", "last", "length", "gaps"):
            empty = -1 if k in ("first", "last") else 0
            assert st["stitch_" + k][s].tolist() == spec[k] + [empty] * (F * T - N), k
        linked = np.array(spec["parent"]) >= 0
        assert (st["stitch_d2"][s, :N][~linked] == 0).all() and (st["stitch_affinity"][s, :N][~linked] == 0).all()
        assert (st["stitch_affinity"][s, :N][linked] > 0).all() and not st["stitch_d2"][s, N:].any()
    ids = out["track_id"]
    want = np.where(ids >= 0, np.array(spec["root"])[np.maximum(ids, 0)], -1)
    assert same(st["stitch_id"], want.astype(np.int32))
    for k in track.STITCH_OUTPUTS:
        assert st[k].dtype == (np.float32 if k in ("stitch_d2", "stitch_affinity") else np.int32), k


def test_optimal_stitching_keeps_both_objects_where_greedy_swaps_them():
    spec, case, out, st = run("TWO_BEHIND", return_state=True)
    assert st["stitch_parent"][0, :4].tolist() == [-1, -1, 0, 1]
    pairs = st["stitch_pairs"]
    assert all(pairs[(0, a, b)][2] is not None for a in (0, 1) for b in (2, 3))      # all four admissible
    assert pairs[(0, 0, 3)][2] > max(pairs[(0, 0, 2)][2], pairs[(0, 1, 3)][2], pairs[(0, 1, 2)][2])      # the best pair is a wrong one
    greedy = SC.greedy_parent(pairs, 0, 4)
    assert greedy == spec["greedy_parent"] == [-1, -1, 1, 0]        # greedy swaps A and B
    total = lambda parent: sum(pairs[(0, a, b)][2] for b, a in enumerate(parent) if a >= 0)
    assert total([-1, -1, 0, 1]) > total(greedy)
    # the ground truth: slot 0 is A, slot 1 is B in every frame; the stitched ids follow the objects
    ids = MC.frame_ids(case, {"track_id": st["stitch_id"]})
    assert all(f == [0, 1] for f in ids if f)


def test_lookalike_equal_d2_and_the_what_rows_decide():
    spec, case, out, st = run("LOOKALIKE", return_state=True)
    p1, p2 = st["stitch_pairs"][(0, 0, 1)], st["stitch_pairs"][(0, 0, 2)]
    assert p1[0] == p2[0] and p1[1] == 1.0 and p2[1] == 0.0 and p2[2] > p1[2]
    assert st["stitch_parent"][0, :3].tolist() == [-1, -1, 0]
    flat = SC.stitch(case, out, appearance_weight=0.0, return_state=True)      # without the `what` term: an exact tie, one link either way
    assert flat["stitch_pairs"][(0, 0, 1)][2] == flat["stitch_pairs"][(0, 0, 2)][2] and flat["num_links"][0] == 1


# ---- 2. the exact consequences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(gate=1e-300), dict(max_gap=1)], ids=["gate_1e-300", "max_gap_1"])
def test_consequence_1_no_admissible_pair_leaves_the_trackers_bits(kw):
    spec, case, out, st = run("LONG_OCCLUSION", S=2, **kw)
    assert not st["num_links"].any() and same(st["stitch_id"], out["track_id"])
    for k in SC.TABLES:
        assert same(st["stitch_" + k[6:]], out[k]), k
    assert (st["stitch_parent"] == -1).all() and st["stitch_root"][:, :2].tolist() == [[0, 1], [0, 1]]
    assert not st["stitch_d2"].any() and not st["stitch_affinity"].any()


def test_consequence_2_restitching_links_nothing_new_in_the_stated_case():
    """LONG_OCCLUSION under max_gap = 8: the one chain has one link, and the stitched output holds no further fragment to reach"""
    spec, case, out, st = run("LONG_OCCLUSION")
    again = track.reference_stitch(case["what"], case["where"], st["stitch_id"], out["num_tracks"], st["stitch_first"], st["stitch_last"],
                                   st["stitch_length"], st["stitch_gaps"], case["F"])
    assert again["num_links"][0] == 0 and same(again["stitch_id"], st["stitch_id"])
    for k in track.STITCH_TABLES:
        assert same(again[k], st[k]), k


@pytest.mark.parametrize("noise", sorted(MC.NOISE))
@pytest.mark.parametrize("name", ["CHAIN", "TWO_BEHIND", "LONG_OCCLUSION"])
def test_the_filter_states_are_the_trackers_own_bit_for_bit(name, noise):
    terms = MC.NOISE[noise]
    spec, case, out, st = run(name, S=2, motion=terms, return_state=True, **terms)
    assert sorted(st["stitch_state"]) == sorted(out["motion_state"]) and len(out["motion_state"]) == 2 * len(spec["parent"])
    for key, want in out["motion_state"].items():
        assert all(same(np.asarray(g), np.asarray(w)) for g, w in zip(st["stitch_state"][key], want)), key


def test_the_filter_states_on_random_tracks_with_gaps():
    case, ref = MC.random_case(4, 3, 2, 9, seed=5, max_age=2)
    out = MC.associate_motion(case, return_state=True, **case["kw"])
    st = SC.stitch(case, out, return_state=True)
    assert (out["track_gaps"] > 0).any() and len(out["motion_state"]) >= 6      # tracks that coasted: the one-by-one predict runs
    for key, want in out["motion_state"].items():
        assert all(same(np.asarray(g), np.asarray(w)) for g, w in zip(st["stitch_state"][key], want)), key
    states = MC.final_states(case, out, 2)                          # and the smoother's forward pass on the same tracks
    for key, (x, v) in states.items():
        assert same(st["stitch_state"][key][0], x) and same(st["stitch_state"][key][1], v), key


def test_d2_is_the_gates_statements_with_m_equal_to_the_gap():
    """an independent chain of trajectory._filter_step for every candidate pair: g = first[b] - last[a] predicts one by one from a's
    filtered state, then the gate's sum with the `where` row of b's first sighting; aff from it and the hand-written msd of 0"""
    t = trajectory.DEFAULTS
    q = np.array([t["process_noise"][1], t["process_noise"][0]] * 2, np.float64)
    seen = 0
    for name in ("LONG_OCCLUSION", "CHAIN", "TWO_BEHIND"):
        spec, case, out, st = run(name, return_state=True)
        assert len(st["stitch_pairs"]) == {"LONG_OCCLUSION": 1, "CHAIN": 2, "TWO_BEHIND": 4}[name]
        for (s, a, b), (got, msd, aff) in st["stitch_pairs"].items():
            filt, fb = st["stitch_state"][(s, a)], int(out["track_first"][s, b])
            for _ in range(fb - int(out["track_last"][s, a])):
                filt = trajectory._filter_step(filt, None, q, t["measurement_noise"])[1]
            jb = int(np.flatnonzero(out["track_id"][:, fb] == b)[0])
            e = case["where"][jb, fb].astype(np.float64) - filt[0]
            sn = filt[2] + t["measurement_noise"]
            d2 = ((e[0] * e[0] / sn[0] + e[1] * e[1] / sn[1]) + e[2] * e[2] / sn[2]) + e[3] * e[3] / sn[3]
            assert got == d2 and msd == 0.0 and aff == 0.75 / (1.0 + d2) + 0.25 / 1.0, (name, a, b)
            if st["stitch_parent"][s, b] == a:
                assert st["stitch_d2"][s, b] == np.float32(d2) and st["stitch_affinity"][s, b] == np.float32(aff)
                seen += 1
    assert seen == 5


# ---- 3. the identity figures ---------------------------------------------------------------------------------------------------------------
def test_stitching_repairs_idf1_and_assa_on_the_long_occlusion():
    spec, case, out, st = run("LONG_OCCLUSION", S=2)
    figures = {}
    for name, ids in (("tracker", out["track_id"]), ("stitched", st["stitch_id"])):
        idf = track.reference_identity(case["boxes"], case["n"], ids, case["gt"], case["F"])
        hota = track.reference_hota(case["boxes"], case["n"], ids, case["gt"], case["F"])
        mot = track.reference_score(case["boxes"], case["n"], ids, case["gt"], case["F"])
        figures[name] = (track.idf_summary(idf["seq_idf"].sum(0))["idf1"],
                         track.hota_summary(hota["seq_hota_i"].sum(0), hota["seq_hota_f"].sum(0)),
                         track.mot_summary(mot["seq_counts"].sum(0), mot["seq_iou"].sum())["id_switches"])
    idf1, hota, idsw = figures["tracker"]
    assert idf1 == 0.5 and hota["assa"] == 0.5 and hota["deta"] == 1.0 and idsw == 2      # a track split in two halves
    idf1, hota, idsw = figures["stitched"]
    assert idf1 == 1.0 and hota["assa"] == 1.0 and hota["deta"] == 1.0 and hota["hota"] == 1.0 and idsw == 0


# ---- 4. the 32-track cap -----------------------------------------------------------------------------------------------------------------------
def test_full_32_tracks_and_overflow_at_33():
    case = SC.full_case(16, 16)
    out = SC.tracked(case, appearance_weight=0.25)
    st = SC.stitch(case, out)
    assert out["num_tracks"][0] == 32 and st["stitch_status"][0] == track.STITCHED and st["num_links"][0] == 16
    assert st["stitch_parent"][0].tolist() == [-1] * 16 + list(range(16)) and st["stitch_root"][0].tolist() == list(range(16)) * 2
    assert st["stitch_length"][0, :32].tolist() == [2] * 16 + [0] * 16 and st["stitch_gaps"][0, :32].tolist() == [1] * 16 + [0] * 16
    case = SC.full_case(17, 16)
    out = SC.tracked(case, appearance_weight=0.25)
    st = SC.stitch(case, out)
    assert out["num_tracks"][0] == 33 and st["stitch_status"][0] == track.STITCH_OVERFLOW and st["num_links"][0] == 0
    assert same(st["stitch_id"], out["track_id"]) and all(same(st["stitch_" + k[6:]], out[k]) for k in SC.TABLES)
    assert (st["stitch_parent"] == -1).all() and st["stitch_root"][0].tolist() == list(range(32))
    assert not st["stitch_d2"].any() and not st["stitch_affinity"].any()


def test_inconsistent_tables_are_clipped_not_followed():
    """tables no tracker writes: the reference clips the frames and N and every output stays inside its ranges"""
    links = 0
    for seed in (1, 2, 3):
        case, tracks = SC.inconsistent_case(seed)
        st = SC.stitch(case, tracks, max_gap=4, gate=1e300)
        S, FT = 6, 18
        assert st["stitch_status"].tolist()[:3] == [1, 0, 0] and ((tracks["num_tracks"] > 32) == (st["stitch_status"] == 1)).all()
        N = np.clip(tracks["num_tracks"], 0, FT)
        for s in range(S):
            if st["stitch_status"][s]:
                assert same(st["stitch_id"][:, s * 9:(s + 1) * 9], tracks["track_id"][:, s * 9:(s + 1) * 9])
                continue
            assert (st["stitch_parent"][s, N[s]:] == -1).all() and (st["stitch_root"][s, N[s]:] == -1).all()
            assert ((st["stitch_root"][s, :N[s]] >= 0) & (st["stitch_root"][s, :N[s]] < max(N[s], 1))).all()
            assert all(same(st["stitch_" + k[6:]][s, N[s]:], tracks[k][s, N[s]:]) for k in SC.TABLES)      # the rows from N on: copied
        links += int(st["num_links"].sum())
    assert links >= 3


# ---- 5. the refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    spec, case, out, _ = run("LONG_OCCLUSION")
    for kw, text in ((dict(max_gap=0), "max_gap"), (dict(max_gap=1.5), "max_gap"), (dict(max_gap=True), "max_gap"),
                     (dict(gate=0.0), "motion_gate"), (dict(gate=float("inf")), "motion_gate"), (dict(gate=float("nan")), "motion_gate"),
                     (dict(gate=None), "needs a gate"), (dict(appearance_weight=1.5), "appearance_weight"),
                     (dict(appearance_weight=-0.1), "appearance_weight"), (dict(measurement_noise=1e-150), "measurement_noise"),
                     (dict(process_noise=(0.0, 1e-4)), "process_noise"), (dict(velocity_var=1e4), "velocity_var")):
        with pytest.raises(ValueError, match=text):
            SC.stitch(case, out, **kw)
    with pytest.raises(ValueError, match="where"):
        track.reference_stitch(case["what"], case["where"][:, :5], out["track_id"], out["num_tracks"], out["track_first"], out["track_last"],
                               out["track_length"], out["track_gaps"], case["F"])
    with pytest.raises(ValueError, match="tables"):
        track.reference_stitch(case["what"], case["where"], out["track_id"], out["num_tracks"], out["track_first"][:, :3], out["track_last"],
                               out["track_length"], out["track_gaps"], case["F"])
    assert track.check_stitch() == (8, track.MOTION_GATE_DEFAULT, 0.25, track.check_motion(True))
    with pytest.raises(ValueError, match="out of scope on a stream"):
        track.TrackStitcher(object.__new__(track.StreamTracker))
    with pytest.raises(ValueError, match="SequenceTracker"):
        track.TrackStitcher(object())


def test_the_key_of_the_track_family_with_stitch():
    from attend_infer_repeat_amd.engine import EngineConfig
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    S, F = 2, 6
    plain = stacks.track_key(eng, S, F)
    assert plain.stitch is None and plain == stacks.track_key(eng, S, F, stitch=None) == stacks.track_key(eng, S, F, stitch=False)
    on = stacks.track_key(eng, S, F, stitch=True)
    assert on != plain and on.stitch == (8, track.MOTION_GATE_DEFAULT, None, None)
    assert on == stacks.track_key(eng, S, F, stitch=8) == stacks.track_key(eng, S, F, stitch=dict(max_gap=8, gate=True))
    others = [stacks.track_key(eng, S, F, stitch=v) for v in (4, dict(gate=9.0), dict(appearance_weight=0.5),
                                                              dict(measurement_noise=1e-3), dict(velocity_var=0.0))]
    assert len(set(others + [on, plain])) == len(others) + 2
    assert dict(others[3].stitch[3]) == dict(track.check_motion(dict(measurement_noise=1e-3)))
    assert stacks.track_key(eng, S, F, stitch=True, temporal=1).stack.temporal == (1, 1)      # a provider: allowed
    with pytest.raises(ValueError, match="stitch= together with smooth="):
        stacks.track_key(eng, S, F, stitch=True, smooth=True)
    for bad in (0, -1, 1.5, "x", dict(gap=1), dict(gate=0.0), dict(appearance_weight=2.0)):
        with pytest.raises(ValueError):
            stacks.track_key(eng, S, F, stitch=bad)
    with pytest.raises(TypeError, match="stitch"):
        stacks.stream_key(eng, S, F, stitch=True)
    with pytest.raises(ValueError, match="stitch= has no part"):
        stacks.fit_key(eng, S, F, stitch=True)
    # the stack: the stitcher bound to the tracker, with the key's arguments
    made = []
    stub = lambda kind: (lambda bound, *a, **kw: made.append((kind, bound, a, kw)) or (kind, len(made)))
    classes = tuple(stub(k) for k in ("tracker", "stream_tracker", "smoother", "stream_smoother", "fitter"))
    key = stacks.track_key(eng, S, F, stitch=dict(max_gap=3, gate=9.0, appearance_weight=0.5), motion=True)
    stack = stacks.build_track_stack(["provider"], key, classes=classes, stitcher=stub("stitcher"))
    assert [m[0] for m in made] == ["tracker", "stitcher"] and made[1][1] == stack[1] and stack[2] == ("stitcher", 2)
    assert made[1][3] == dict(max_gap=3, gate=9.0, appearance_weight=0.5, noise=None)
    assert len(stacks.build_track_stack(["provider"], plain, classes=classes, stitcher=stub("stitcher"))) == 2


def test_the_header_the_ctypes_table_and_the_launch_tuple_agree():
    import ctypes
    import os
    import re
    from attend_infer_repeat_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "air_hip.h")).read(), flags=re.S)
    m = re.search(r"AIR_ENGINE_API int air_track_stitch\(([^;]*)\);", src)
    decl = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", d).group(1) for d in decl]
    assert names[-1] == "stream" and tuple(names[:-1]) == track.STITCH_ARGS
    sig = _lib.SIGNATURES["air_track_stitch"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == len(decl)
    for d, c in zip(decl, sig[1]):
        assert c is (_lib.P if "*" in d else (ctypes.c_double if d.startswith("double") else ctypes.c_int)), d


# ---- 6. the planted defects of the reference -------------------------------------------------------------------------------------------------
def scenario_checks():
    """the checks of sections 1 and 2 a defect has to get past, as one function: the hand-written tables, the independent d2, a gate
    set exactly at a pair's d2"""
    for name in sorted(SC.SCENARIOS):
        for motion in (None, {}):
            test_the_scenarios_by_hand(name, motion)
    test_d2_is_the_gates_statements_with_m_equal_to_the_gap()
    test_a_gate_equal_to_d2_admits_the_pair()


def test_a_gate_equal_to_d2_admits_the_pair():
    spec, case, out, st = run("LONG_OCCLUSION", return_state=True)
    d2 = st["stitch_pairs"][(0, 0, 1)][0]
    at = SC.stitch(case, out, gate=d2, return_margins=True)
    assert at["num_links"][0] == 1 and at["gate_margin"][0] == 0.0
    below = SC.stitch(case, out, gate=np.nextafter(d2, 0.0), return_margins=True)
    assert below["num_links"][0] == 0 and 0.0 < below["gate_margin"][0] < 1e-18


def test_the_rule_itself_passes_the_checks():
    with SC.planted(None):
        scenario_checks()


@pytest.mark.parametrize("defect", SC.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    with SC.planted(defect):
        with pytest.raises(AssertionError):
            scenario_checks()
    scenario_checks()                                              # and the rule is back


@pytest.mark.parametrize("defect,name", [("first_sighting_of_a", "TOO_FAR"), ("gaps_without_the_link", "CHAIN"), ("gaps_without_the_link", "LONG_OCCLUSION")])
def test_which_scenario_catches_which_defect(defect, name):
    with SC.planted(defect):
        with pytest.raises(AssertionError):
            test_the_scenarios_by_hand(name, None)


def test_gv_and_the_strict_gate_are_caught_by_their_own_checks():
    with SC.planted("gv_for_the_prediction"):
        with pytest.raises(AssertionError):
            test_d2_is_the_gates_statements_with_m_equal_to_the_gap()
    with SC.planted("strict_gate"):
        with pytest.raises(AssertionError):
            test_a_gate_equal_to_d2_admits_the_pair()


# ---- 7. the random batches of the device test: conditions, not measurements ----------------------------------------------------------------
def test_the_random_batches_link_refuse_by_the_gate_and_refuse_by_max_gap():
    """the device test compares every output of these batches bit for bit; it must not pass vacuously: the reference itself links,
    refuses candidates by the gate and leaves pairs beyond max_gap, and tracks with a non-finite `where` value take part"""
    links = refused = late = nonfinite = 0
    planted_nonfinite = False                                      # by the case builder: NaN / inf in `where` and in `what` of one batch
    for p in SC.RANDOM:
        T, A, S, F = p[:4]
        assert T <= 4 and F <= 12 and S <= 4 and A in (2, 8, 50)
        case, ref = SC.random_case(*p)
        planted_nonfinite = planted_nonfinite or (not np.isfinite(case["where"]).all() and not np.isfinite(case["what"]).all())
        st = SC.stitch(case, ref, return_state=True, **SC.RANDOM_STITCH)
        assert (st["stitch_status"] == 0).all() and (ref["num_tracks"] <= 32).all()
        links += int(st["num_links"].sum())
        refused += sum(1 for v in st["stitch_pairs"].values() if v[2] is None and np.isfinite(v[0]))
        nonfinite += sum(1 for v in st["stitch_pairs"].values() if not np.isfinite(v[0]))
        for s in range(S):
            N = int(ref["num_tracks"][s])
            gap = ref["track_first"][s, :N][None, :] - ref["track_last"][s, :N][:, None]
            late += int((gap > SC.RANDOM_STITCH["max_gap"]).sum())
            assert (st["stitch_parent"][s, :N] >= 0).sum() == st["num_links"][s]
            for b in np.flatnonzero(st["stitch_parent"][s] >= 0):
                a = int(st["stitch_parent"][s, b])
                assert 1 <= ref["track_first"][s, b] - ref["track_last"][s, a] <= SC.RANDOM_STITCH["max_gap"]
    print("links", links, "refused by the gate", refused, "beyond max_gap", late, "non-finite d2", nonfinite)
    assert links >= 10 and refused >= 10 and late >= 10 and nonfinite >= 1 and planted_nonfinite
