"""Host-side tests of motion-predicted association (track.reference_associate_motion alone): the occlusion and crossing scenarios
against the ids written out by hand, the two exact consequences of the rule, the refusals, and planted defects.  No GPU."""
import numpy as np
import pytest

import track_motion_cases as MC
from attend_infer_repeat_amd import track, trajectory

bits = lambda a: np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b, keys, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def idsw(case, out):
    return int(track.reference_score(case["boxes"], case["n"], out["track_id"], case["gt"], case["F"])["seq_counts"][:, 4].sum())


# ---- 1. the scenarios -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("name", ["OCCLUSION", "CROSSING"])
def test_motion_keeps_the_identity_the_last_box_rule_loses(name, matching):
    spec = getattr(MC, name)
    case = MC.scenario(spec)
    kw = dict(MC.KW, max_age=spec["max_age"], matching=matching)
    motion, last_box = MC.associate_motion(case, return_margins=True, **kw), MC.associate_last_box(case, return_margins=True, **kw)
    assert MC.frame_ids(case, motion) == spec["ids"]
    assert MC.frame_ids(case, last_box) == spec["ids_last_box"]
    assert idsw(case, motion) == 0
    assert idsw(case, last_box) >= 1                               # (or the scenario has quietly stopped discriminating)
    # no decision sits on a rounding: the smallest |iou - iou_gate| over the pairs of step 2.  Measured 0.1 under both rules and
    # both matchings in both scenarios (a pair without overlap against the gate 0.1; the closest overlapping pair is 0.15 away):
    # the threshold is that measured margin / 10
    margin = min(float(motion["gate_margin"].min()), float(last_box["gate_margin"].min()))
    print("\n  %s %s: gate margin %.6g" % (name, matching, margin))
    assert margin >= 0.1 / 10


@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_an_object_too_fast_from_birth_is_not_linked_by_either_rule(matching):
    """a track has v = 0 until its second sighting: its first prediction is its last box.  Documented, not a defect."""
    case = MC.scenario(MC.FAST)
    kw = dict(MC.KW, max_age=MC.FAST["max_age"], matching=matching)
    motion, last_box = MC.associate_motion(case, **kw), MC.associate_last_box(case, **kw)
    assert MC.frame_ids(case, motion) == MC.frame_ids(case, last_box) == MC.FAST["ids"]
    same_bits(motion, last_box, MC.OUTPUTS)


def test_pred_rows_are_the_prediction_of_the_matched_track_and_zero_elsewhere():
    case = MC.scenario(MC.OCCLUSION)
    out = MC.associate_motion(case, max_age=2, **MC.KW)
    matched = out["obj_state"] == track.MATCHED
    assert not out["pred_where"][~matched].any() and not out["pred_boxes"][~matched].any()
    # frame 6 after the sightings 0..3 of a constant rate 0.24: the prediction has moved on by about three frames from the last row
    assert abs(float(out["pred_where"][0, 6, 1]) - (-0.6 + 0.24 * 6)) < 0.02
    assert np.array_equal(out["pred_where"][0, 6, [0, 2, 3]], case["where"][0, 3, [0, 2, 3]])      # scales (and a still ty) held
    assert np.array_equal(out["pred_boxes"][0, 6], MC.scene_boxes(out["pred_where"][0, 6], case["img"]))
    assert np.array_equal(out["pred_where"][0, 1], case["where"][0, 0])                            # v = 0 after the birth


# ---- 2. exact consequence 1: zero velocity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_static_tracks_give_the_bits_of_the_last_box_rule(matching):
    case = MC.scenario(MC.STATIC, S=2)
    kw = dict(MC.KW, max_age=1, matching=matching)
    same_bits(MC.associate_motion(case, **kw), MC.associate_last_box(case, **kw), MC.OUTPUTS)
    for seed in range(3):
        case, ref = MC.random_case(4, 3, 2, 7, seed=seed, max_age=2, matching=matching, static=True, bad=False)
        assert (ref["obj_state"] == track.MATCHED).sum() >= 5
        same_bits(ref, MC.associate_last_box(case, **{k: v for k, v in case["kw"].items()}), MC.OUTPUTS, seed)
        matched = ref["obj_state"] == track.MATCHED
        prev = case["where"][ref["prev_slot"][matched], np.nonzero(matched)[1] - (np.nonzero(matched)[1] % 7) + ref["prev_frame"][matched]]
        assert np.array_equal(bits(ref["pred_where"][matched]), bits(prev))      # the prediction is the last `where` row


@pytest.mark.parametrize("matching", track.MATCHINGS)
@pytest.mark.parametrize("F", [1, 2])
def test_two_frames_or_fewer_give_the_bits_of_the_last_box_rule_on_any_rows(F, matching):
    rng = np.random.default_rng(F)
    T, A, S = 5, 3, 4
    what, where = rng.normal(size=(T, S * F, A)).astype(np.float32), rng.uniform(-1, 1, (T, S * F, 4)).astype(np.float32)
    where[..., [0, 2]] = rng.uniform(0.3, 0.9, (T, S * F, 2))      # large boxes: many pairs pass the gate
    case = dict(what=what, where=where, boxes=MC.scene_boxes(where, MC.IMG), score=rng.uniform(size=(T, S * F)).astype(np.float32),
                n=rng.integers(0, T + 1, S * F).astype(np.int32), F=F, img=MC.IMG)
    kw = dict(max_age=1, matching=matching)
    motion, last_box = MC.associate_motion(case, **kw), MC.associate_last_box(case, **kw)
    assert F == 1 or (motion["obj_state"] == track.MATCHED).sum() >= 4
    same_bits(motion, last_box, MC.OUTPUTS)


# ---- 3. exact consequence 2: one filter --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", sorted(MC.NOISE))
@pytest.mark.parametrize("matching", track.MATCHINGS)
def test_the_prediction_is_the_smoothers_forecast_on_the_truncated_tables(matching, noise):
    terms = MC.NOISE[noise]
    case, ref = MC.random_case(4, 3, 2, 9, seed=2, max_age=3, matching=matching, noise=terms)
    pairs = MC.smoother_forecasts(case, ref, 3, terms)
    coasted = ref["prev_frame"][ref["obj_state"] == track.MATCHED] + 1 < (np.nonzero(ref["obj_state"] == track.MATCHED)[1] % 9)
    assert len(pairs) >= 15 and coasted.sum() >= 2                 # matches, and matches behind a gap
    for mine, smoothers in pairs:
        assert np.array_equal(bits(mine), bits(smoothers))
    # and the float64 state itself is the forward pass of the smoother on the same track
    out = MC.associate_motion(case, return_state=True, **case["kw"])
    expect = MC.final_states(case, out, 3, terms)
    assert set(expect) == set(out["motion_state"])
    for key, (x, v) in expect.items():
        assert np.array_equal(bits(out["motion_state"][key][0]), bits(x)) and np.array_equal(bits(out["motion_state"][key][1]), bits(v))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms, match", [
    (dict(measurement_noise=1e-150), "R_MIN"), (dict(process_noise=(1e-40, 1e-4)), "Q_OVER_R_MIN"),
    (dict(process_noise=(1e-4, 1e13)), "Q_OVER_R_MAX"), (dict(velocity_var=1e4), "V_OVER_R_MAX"),
    (dict(process_noise=(0.0, 1e-4)), "two positive numbers"), (dict(measurement_noise=float("nan")), "positive number"),
    (dict(velocity_var=-1.0), ">= 0")])
def test_noise_outside_the_smoothers_domain_is_refused_with_its_messages(terms, match):
    case = MC.scenario(MC.STATIC)
    with pytest.raises(ValueError, match=match):
        MC.associate_motion(case, **terms)
    with pytest.raises(ValueError, match=match):
        track.check_motion(terms)
    with pytest.raises(ValueError, match=match):                   # the smoother's own check says the same
        trajectory.check_arguments(2, 5, **terms)


@pytest.mark.parametrize("motion, match", [
    (dict(q=1.0), "unknown keys"), ("on", "None, True or a dict"), (3, "None, True or a dict"), (dict(process_noise=1e-4), "two positive"),
    ({1: 2}, "unknown keys")])
def test_a_malformed_motion_setting_is_refused(motion, match):
    with pytest.raises(ValueError, match=match):
        track.check_motion(motion)


def test_check_motion_fills_in_the_defaults():
    assert track.check_motion(None) is None and track.check_motion(False) is None
    full = track.check_motion(True)
    assert full == dict(process_noise=tuple(trajectory.DEFAULTS["process_noise"]), measurement_noise=trajectory.DEFAULTS["measurement_noise"],
                        velocity_var=trajectory.DEFAULTS["velocity_var"])
    assert track.check_motion(dict(velocity_var=0.0)) == dict(full, velocity_var=0.0)


def test_motion_on_a_stream_is_refused():
    """the carried state would need the 14 doubles per slot: a follow-up of its own.  The refusal comes before anything is bound."""
    with pytest.raises(ValueError, match="motion.*stream"):
        track.StreamTracker(object(), 4, motion=True)
    with pytest.raises(ValueError, match="motion.*stream"):
        track.StreamTracker(object(), 4, motion=dict(velocity_var=0.0))


def test_the_shape_of_where_and_the_image_are_checked():
    case = MC.scenario(MC.STATIC)
    with pytest.raises(ValueError, match="where"):
        MC.associate_motion(dict(case, where=case["where"][:, :-1]))
    with pytest.raises(ValueError, match="img_size"):
        MC.associate_motion(dict(case, img=(0, 50)))


# ---- 5. planted defects ------------------------------------------------------------------------------------------------------------------------
def _checks():
    """the checks of this file that a defect of the rule has to trip, each a function that raises AssertionError"""
    def scenarios():
        for name in ("OCCLUSION", "CROSSING"):
            spec = getattr(MC, name)
            case = MC.scenario(spec)
            assert MC.frame_ids(case, MC.associate_motion(case, max_age=spec["max_age"], **MC.KW)) == spec["ids"]

    def one_filter():
        case, ref = MC.random_case(4, 3, 2, 9, seed=2, max_age=3)
        out = MC.associate_motion(case, return_state=True, **case["kw"])
        for mine, smoothers in MC.smoother_forecasts(case, out, 3):
            assert np.array_equal(bits(mine), bits(smoothers))
        for key, (x, v) in MC.final_states(case, out, 3).items():
            assert np.array_equal(bits(out["motion_state"][key][0]), bits(x)) and np.array_equal(bits(out["motion_state"][key][1]), bits(v))

    return dict(scenarios=scenarios, one_filter=one_filter)


def test_without_a_defect_every_check_passes():
    with MC.planted(None):
        for check in _checks().values():
            check()


@pytest.mark.parametrize("defect", MC.DEFECTS)
def test_a_planted_defect_fails_a_check(defect):
    caught = []
    with MC.planted(defect):
        for name, check in _checks().items():
            try:
                check()
            except AssertionError:
                caught.append(name)
    print("\n  %s: caught by %s" % (defect, ", ".join(caught) or "nothing"))
    assert caught
    clean = MC.associate_motion(MC.scenario(MC.OCCLUSION), max_age=2, **MC.KW)      # the planting is undone
    assert MC.frame_ids(MC.scenario(MC.OCCLUSION), clean) == MC.OCCLUSION["ids"]


# ---- 6. the keys of the cached stacks ----------------------------------------------------------------------------------------------------------
def test_the_tracker_cache_key_includes_the_motion_setting():
    import types
    from attend_infer_repeat_amd import stacks
    from attend_infer_repeat_amd.engine_config import EngineConfig
    eng = types.SimpleNamespace(cfg=EngineConfig(), device="cuda:0")
    key = stacks.track_key(eng, 2, 5)
    assert key.motion is None and key == stacks.track_key(eng, 2, 5, motion=None) == stacks.track_key(eng, 2, 5, motion=False)
    on = stacks.track_key(eng, 2, 5, motion=True)
    assert on != key and hash(on) != hash(key) and dict(on.motion) == track.check_motion(True) and on == stacks.track_key(eng, 2, 5, motion={})
    assert stacks.track_key(eng, 2, 5, motion=dict(velocity_var=0.0)) != on
    terms = dict(process_noise=(2e-4, 1e-4), measurement_noise=5e-4, velocity_var=0.01)
    assert dict(stacks.track_key(eng, 2, 5, motion=True, smooth=terms).motion) == track.check_motion(terms)      # the smoother's terms
    assert dict(stacks.track_key(eng, 2, 5, motion=dict(velocity_var=0.02), smooth=terms).motion)["velocity_var"] == 0.02      # an explicit dict wins
    assert stacks.fit_key(eng, 2, 5, motion=True).motion == on.motion and stacks.fit_key(eng, 2, 5).motion is None
    with pytest.raises(ValueError, match="motion.*stream"):
        stacks.stream_key(eng, 2, 5, motion=True)
    with pytest.raises(ValueError, match="motion.*stream"):
        stacks.stream_smoother_key(eng, 2, 5, motion=True)
    with pytest.raises(ValueError, match="Q_OVER_R_MIN"):
        stacks.track_key(eng, 2, 5, motion=dict(process_noise=(1e-40, 1e-4)))
