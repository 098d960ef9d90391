"""Host-side tests of the Mahalanobis gate of motion-predicted association (track.reference_associate_motion(gate=) alone): the
scenarios against the ids and d2 values written out by hand, the two exact consequences, the refusals, the cache keys and planted
defects.  No GPU.

Bars.  The ids are exact.  The d2 values are compared with the figures the rule was worked out to by hand, at the significant digits
those figures were written with (three: 8.82, 15.7, 12.0; two: 0.12, 0.00037, 0.98); pred_d2 against trajectory._filter_step and the
final states against the smoother's forward pass by bits -- so every pred_d2 is also held to far more than three digits."""
import numpy as np
import pytest

import track_gate_cases as GC
import track_motion_cases as MC
from attend_infer_repeat_amd import track, trajectory

bits = lambda a: np.ascontiguousarray(a).view(np.uint8)


def sig(x, want, digits=3):
    """x rounds to `want` at `digits` significant digits: within half a unit of the last of them"""
    unit = 10.0 ** (np.floor(np.log10(abs(want))) - (digits - 1))
    return abs(x - want) <= 0.5 * unit * (1 + 1e-9)


# ---- 1. the scenarios ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("name", sorted(GC.SCENARIOS))
def test_the_ids_of_the_scenarios_under_the_gate(name, matching):
    spec = GC.SCENARIOS[name]
    case, out = GC.scenario_out(name, matching)
    assert MC.frame_ids(case, out) == spec["ids"]
    plain = MC.associate_motion(case, max_age=spec["max_age"], matching=matching, **MC.KW)
    assert MC.frame_ids(case, plain) == spec["ids_iou_gate"]       # (the rule without the gate: what the gate changes, or does not)
    assert "pred_d2" not in plain and out["pred_d2"].dtype == np.float32 and out["pred_d2"].shape == out["track_id"].shape
    assert not out["pred_d2"][out["obj_state"] != track.MATCHED].any()


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_the_d2_values_of_the_scenarios(matching):
    case, out = GC.scenario_out("FAST", matching)
    d2 = out["pred_d2"][0]
    print("\n  FAST d2", d2.tolist())
    assert sig(d2[1], 8.82) and sig(d2[2], 0.12, 2)                 # a newborn track's rate is unknown: 15 px in one step is 8.82
    case, out = GC.scenario_out("OCCLUSION", matching)
    print("  OCCLUSION d2", out["pred_d2"][0].tolist())
    assert sig(out["pred_d2"][0, 6], 0.00037, 2)                     # after the two unseen frames
    # CROSSING: the right pair at most 0.98, the wrong pair at least 15.7, in every frame
    case, out = GC.scenario_out("CROSSING", matching)
    right = out["pred_d2"][:, 1:]
    wrong = np.array([[GC.pair_d2(case, out, f, 1 - j, j, 1) for f in range(1, case["F"])] for j in range(2)])
    print("  CROSSING right max %.4g wrong min %.4g" % (right.max(), wrong.min()))
    assert (out["obj_state"][:, 1:] == track.MATCHED).all() and right.max() <= 0.98 and sig(right.max(), 0.98, 2)
    assert sig(wrong.min(), 15.7) and wrong.min() > GC.GATE      # (15.68: "at least 15.7" is that figure at three digits)
    # STATIC: at frame 1 both newborn tracks have an unknown rate and a wrong pair is admissible (12.0 < the gate): the ranking decides
    case, out = GC.scenario_out("STATIC", matching)
    wrong = [GC.pair_d2(case, out, 1, 1 - j, j, 1) for j in range(2)]
    print("  STATIC wrong pairs at frame 1", wrong)
    assert sig(min(wrong), 12.0) and min(wrong) < GC.GATE and not out["pred_d2"].any()      # the right pairs: d2 = 0 exactly


def test_clutter_lies_outside_the_gate_and_not_on_it():
    case, out = GC.scenario_out("CLUTTER", return_margins=True)
    d2 = GC.pair_d2(case, out, 6, 0, 0, 2)                         # B against A's track, coasting since frame 5
    print("\n  CLUTTER: d2 of B %.9g, the gate %.9g, gate margin %.6g" % (d2, GC.GATE, float(out["gate_margin"][0])))
    # d2 of B = 13.3386770 (this rule at the default noise terms): 0.062 outside the gate
    assert d2 > GC.GATE and abs(d2 - GC.GATE) >= 1e-6 and float(out["gate_margin"][0]) >= 1e-6
    assert np.isclose(float(out["gate_margin"][0]), d2 - GC.GATE, rtol=0, atol=1e-12)      # the closest decision of the scenario is B's
    near, out_near = GC.scenario_out(GC.CLUTTER_NEAR, return_margins=True)
    assert MC.frame_ids(near, out_near) == GC.CLUTTER_NEAR["ids"] and out_near["pred_d2"][0, 6] < GC.GATE
    assert float(out_near["gate_margin"][0]) >= 1e-6
    assert MC.frame_ids(near, MC.associate_motion(near, max_age=2, **MC.KW)) == GC.CLUTTER_NEAR["ids_iou_gate"]


# ---- 2. the exact consequences --------------------------------------------------------------------------------------------------------------
def consequences(matching, noise):
    terms = MC.NOISE[noise]
    case, ref = MC.random_case(4, 3, 2, 9, seed=2, max_age=3, matching=matching, noise=terms, gate=GC.GATE)
    matched = ref["obj_state"] == track.MATCHED
    coasted = ref["prev_frame"][matched] + 1 < (np.nonzero(matched)[1] % 9)
    assert matched.sum() >= 12 and coasted.sum() >= 1, (matched.sum(), coasted.sum())      # matches, and matches behind a gap
    # 1. pred_d2 is float32(sum e^2 / s) of trajectory._filter_step's predicted tuple
    pairs = GC.matched_d2(case, ref, 3, terms)
    assert len(pairs) == matched.sum()
    for mine, steps in pairs:
        assert np.array_equal(bits(mine), bits(steps)), (mine, steps)
    assert (ref["pred_d2"][matched] <= np.float32(GC.GATE)).all() and (ref["pred_d2"][matched] > 0).any()
    # 2. one filter: pred_where is the smoother's forecast, the final states its forward pass
    for mine, smoothers in MC.smoother_forecasts(case, ref, 3, terms):
        assert np.array_equal(bits(mine), bits(smoothers))
    out = GC.associate_gated(case, return_state=True, **{k: v for k, v in case["kw"].items() if k != "gate"})
    expect = MC.final_states(case, out, 3, terms)
    assert set(expect) == set(out["motion_state"])
    for key, (x, v) in expect.items():
        assert np.array_equal(bits(out["motion_state"][key][0]), bits(x)) and np.array_equal(bits(out["motion_state"][key][1]), bits(v))


@pytest.mark.parametrize("noise", sorted(MC.NOISE))
@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_pred_d2_is_the_filters_innovation_and_the_states_are_the_smoothers(matching, noise):
    consequences(matching, noise)


def test_without_the_gate_the_reference_is_the_motion_rule():
    case, ref = MC.random_case(4, 3, 2, 9, seed=2, max_age=3)
    for off in (None, False):
        again = MC.associate_motion(case, gate=off, **case["kw"])
        assert set(again) == set(MC.MOTION_OUTPUTS)
        for k in MC.MOTION_OUTPUTS:
            assert np.array_equal(bits(again[k]), bits(ref[k])), k


def test_the_gate_replaces_the_iou_gate_and_the_affinity_is_rational():
    case, out = GC.scenario_out("FAST")
    assert (np.abs(np.diff(case["boxes"][0, :, 0])) > case["boxes"][0, 0, 2]).all()      # no overlap between consecutive sightings
    d2 = GC.pair_d2(case, out, 1, 0, 0, 1)
    assert np.array_equal(bits(out["affinity"][0, 1]), bits(np.float32(1.0 / (1.0 + d2))))      # w = 0: aff = 1 / (1 + d2)
    w = 0.25
    _, mixed = GC.scenario_out("FAST", appearance_weight=w)        # what = 0: msd = 0
    assert np.array_equal(bits(mixed["affinity"][0, 1]), bits(np.float32((1.0 - w) / (1.0 + d2) + w / 1.0)))
    # a tiny gate links nothing, a huge gate everything that is finite
    _, none = GC.scenario_out("OCCLUSION", gate=1e-300)
    assert not (none["obj_state"] == track.MATCHED).any()
    _, every = GC.scenario_out("FAST", gate=1e300)
    assert MC.frame_ids(case, every) == [[0], [0], [0]]


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "wide", (1.0,)])
def test_a_gate_that_is_no_positive_finite_number_is_refused(gate):
    with pytest.raises(ValueError, match="motion_gate"):
        track.check_motion_gate(gate, True)
    with pytest.raises(ValueError, match="motion_gate"):
        GC.associate_gated(MC.scenario(MC.STATIC), gate)


def test_check_motion_gate():
    on = track.check_motion(True)
    assert track.check_motion_gate(None, on) is None and track.check_motion_gate(False, on) is None
    assert track.check_motion_gate(None, None) is None and track.check_motion_gate(False, None) is None
    assert track.check_motion_gate(True, on) == track.MOTION_GATE_DEFAULT == 13.2767 == GC.GATE
    assert track.check_motion_gate(9, on) == 9.0 and isinstance(track.check_motion_gate(9, on), float)
    assert track.check_motion_gate(np.float32(2.5), True) == 2.5
    for motion in (None, False):
        with pytest.raises(ValueError, match="needs motion"):
            track.check_motion_gate(True, motion)
        with pytest.raises(ValueError, match="needs motion"):
            track.check_motion_gate(5.0, motion)


def test_the_gate_on_a_stream_is_refused():
    """with the wording of motion on a stream, before anything is bound"""
    for kw in (dict(motion_gate=True), dict(motion_gate=5.0), dict(motion=True, motion_gate=True)):
        with pytest.raises(ValueError, match="motion.*stream"):
            track.StreamTracker(object(), 4, **kw)


# ---- 4. the keys of the cached stacks ------------------------------------------------------------------------------------------------------------
def test_the_cache_keys_include_the_gate():
    import types
    from attend_infer_repeat_amd import stacks
    from attend_infer_repeat_amd.engine_config import EngineConfig
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    plain, motion = stacks.track_key(eng, 2, 5), stacks.track_key(eng, 2, 5, motion=True)
    assert plain.motion_gate is None and motion.motion_gate is None
    assert motion == stacks.track_key(eng, 2, 5, motion=True, motion_gate=None) == stacks.track_key(eng, 2, 5, motion=True, motion_gate=False)
    gated = stacks.track_key(eng, 2, 5, motion=True, motion_gate=True)
    assert gated != motion and hash(gated) != hash(motion) and gated.motion_gate == track.MOTION_GATE_DEFAULT and gated.motion == motion.motion
    assert gated == stacks.track_key(eng, 2, 5, motion=True, motion_gate=13.2767) != stacks.track_key(eng, 2, 5, motion=True, motion_gate=9.0)
    assert stacks.fit_key(eng, 2, 5, motion=True, motion_gate=True).motion_gate == track.MOTION_GATE_DEFAULT
    assert stacks.fit_key(eng, 2, 5, motion=True).motion_gate is None and stacks.fit_key(eng, 2, 5).motion_gate is None
    with pytest.raises(ValueError, match="needs motion"):
        stacks.track_key(eng, 2, 5, motion_gate=True)
    with pytest.raises(ValueError, match="motion_gate"):
        stacks.track_key(eng, 2, 5, motion=True, motion_gate=0.0)
    for kw in (dict(motion_gate=True), dict(motion=True, motion_gate=True)):
        with pytest.raises(ValueError, match="motion.*stream"):
            stacks.stream_key(eng, 2, 5, **kw)
        with pytest.raises(ValueError, match="motion.*stream"):
            stacks.stream_smoother_key(eng, 2, 5, **kw)
    assert stacks.stream_key(eng, 2, 5, motion_gate=None) == stacks.stream_key(eng, 2, 5) == stacks.stream_key(eng, 2, 5, motion_gate=False)


# ---- 5. planted defects ------------------------------------------------------------------------------------------------------------------------
def _checks():
    """the checks of this file that a defect of the gated rule has to trip, each a function that raises AssertionError"""
    def scenarios():
        for name, spec in GC.SCENARIOS.items():
            case, out = GC.scenario_out(name)
            assert MC.frame_ids(case, out) == spec["ids"], name

    def values():
        test_the_d2_values_of_the_scenarios("greedy")

    def innovation():
        consequences("greedy", "defaults")

    def innovation_two_classes():                                  # q_shift != q_scale: the two classes have different s
        consequences("greedy", "loose")

    def affinity():
        test_the_gate_replaces_the_iou_gate_and_the_affinity_is_rational()

    return dict(scenarios=scenarios, values=values, innovation=innovation, innovation_two_classes=innovation_two_classes, affinity=affinity)


def test_without_a_defect_every_check_passes():
    with GC.planted(None):
        for check in _checks().values():
            check()


@pytest.mark.parametrize("defect", GC.DEFECTS)
def test_a_planted_defect_fails_a_check(defect):
    caught = []
    with GC.planted(defect):
        for name, check in _checks().items():
            try:
                check()
            except AssertionError:
                caught.append(name)
    print("\n  %s: caught by %s" % (defect, ", ".join(caught) or "nothing"))
    assert caught
    if defect == "iou_gate_still_applied":
        assert "scenarios" in caught                               # FAST: its sightings do not overlap
    case, clean = GC.scenario_out("FAST")                          # the planting is undone
    assert MC.frame_ids(case, clean) == GC.FAST["ids"]
