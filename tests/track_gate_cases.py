"""Cases shared by test_track_gate_host.py and test_track_gate.py: the scenarios of track_motion_cases under the Mahalanobis gate with
the ids and d2 values written out, the CLUTTER scenario, the numpy restatement of exact consequence 1 (pred_d2 from
trajectory._filter_step alone) and the planted defects of the gated rule."""
import contextlib

import numpy as np

import track_motion_cases as MC
from attend_infer_repeat_amd import track, trajectory

GATE = 13.2767                                                     # the 0.99 quantile of chi-squared with 4 degrees of freedom
GATED_OUTPUTS = MC.MOTION_OUTPUTS + ("pred_d2",)

# A is (0.2, -0.6 + 0.1 f, 0.2, 0) and gone in frames 6 and 7; B sits 0.12 off A's path in frame 6 only.  A track followed for six
# frames has a tight prediction: B overlaps its predicted box (the IoU rule links it) and lies outside the gate.  At 0.08 both link.
_clutter = lambda off: dict(objects=[MC._obj(lambda f: -0.6 + 0.1 * f, gone=(6, 7)), lambda f: (0.2, off, 0.2, 0.0) if f == 6 else None],
                            F=8, T=1, max_age=2)
CLUTTER = dict(_clutter(0.12), ids=[[0]] * 6 + [[1], []], ids_iou_gate=[[0]] * 7 + [[]])
CLUTTER_NEAR = dict(_clutter(0.08), ids=[[0]] * 7 + [[]], ids_iou_gate=[[0]] * 7 + [[]])
# the ids under the gate (default noise terms, appearance_weight 0, either matching) and, where the rule without the gate differs, its
FAST = dict(MC.FAST, ids=[[0], [0], [0]], ids_iou_gate=MC.FAST["ids"])
OCCLUSION = dict(MC.OCCLUSION, ids_iou_gate=MC.OCCLUSION["ids"])
CROSSING = dict(MC.CROSSING, ids_iou_gate=MC.CROSSING["ids"])
STATIC = dict(MC.STATIC, ids=[[0, 1], [0, 1], [0], [0, 1], [0, 1]], ids_iou_gate=[[0, 1], [0, 1], [0], [0, 1], [0, 1]])
SCENARIOS = dict(FAST=FAST, OCCLUSION=OCCLUSION, CROSSING=CROSSING, STATIC=STATIC, CLUTTER=CLUTTER)


def associate_gated(case, gate=GATE, **kw):
    return MC.associate_motion(case, gate=gate, **kw)


def scenario_out(name, matching="greedy", gate=GATE, **kw):
    spec = SCENARIOS[name] if isinstance(name, str) else name
    case = MC.scenario(spec)
    return case, associate_gated(case, gate, max_age=spec["max_age"], matching=matching, **dict(MC.KW, **kw))


def pair_d2(case, out, f, k_id, j, max_age, noise=None, s=0):
    """d2 of the pair (track with id k_id, object j of frame f) of sequence s, from the tracker's own output before f and
    trajectory._filter_start / _filter_step alone: the filter run over the track's sightings (None where it coasted), the frames
    coasted over up to f - 1 predicted one by one, then the predicted tuple of one more step"""
    terms = dict(trajectory.DEFAULTS, **(noise or {}))
    (q_shift, q_scale), r, vv = terms["process_noise"], terms["measurement_noise"], terms["velocity_var"]
    q = np.array([q_scale, q_shift, q_scale, q_shift], np.float64)
    F, T = case["F"], case["T"]
    filt = None
    with np.errstate(all="ignore"):
        for g in range(f):
            col = s * F + g
            hit = [i for i in range(int(np.clip(case["n"][col], 0, T))) if out["track_id"][i, col] == k_id]
            z = case["where"][hit[0], col].astype(np.float64) if hit else None
            if filt is None:
                if z is not None:
                    filt = trajectory._filter_start(z, r, vv)
                continue
            filt = trajectory._filter_step(filt, z, q, r)[1]
        assert filt is not None, (f, k_id)
        xp, _, Pxxp = trajectory._filter_step(filt, None, q, r)[0][:3]
        e = case["where"][j, s * F + f].astype(np.float64) - xp
        return float(np.cumsum(e * e / (Pxxp + r))[-1])


def matched_d2(case, out, max_age, noise=None):
    """[(pred_d2 of the tracker, float32 of pair_d2)] over every MATCHED object: exact consequence 1"""
    pairs = []
    for s in range(case["S"]):
        for f in range(case["F"]):
            r = s * case["F"] + f
            for j in range(int(np.clip(case["n"][r], 0, case["T"]))):
                if out["obj_state"][j, r] == track.MATCHED:
                    pairs.append((out["pred_d2"][j, r], np.float32(pair_d2(case, out, f, out["track_id"][j, r], j, max_age, noise, s))))
    return pairs


# ---- the planted defects of the gated rule ---------------------------------------------------------------------------------------------
DEFECTS = ("s_without_r", "shifts_only", "classes_swapped", "iou_gate_still_applied", "iou_in_the_affinity")


@contextlib.contextmanager
def planted(defect):
    """track.reference_associate_motion(gate=) with one statement of the gated rule replaced (None: the rule itself)"""
    state, d2, pair = track._motion_predicted_state, track._motion_d2, track._gated_pair

    def bad_state(filt, m, q, r):
        xp, s = state(filt, m, q, r)
        return xp, s - r                                           # s_without_r (the sum undone: to a rounding, far from r itself)

    def bad_d2(xp, s, z):
        e = z - xp
        if defect == "shifts_only":
            return e[1] * e[1] / s[1] + e[3] * e[3] / s[3]
        return d2(xp, s[[1, 0, 3, 2]], z)                          # classes_swapped

    def bad_pair(dd, msd, w, gate, pred_box, box):
        iou = track.box_iou(pred_box, box)
        if defect == "iou_gate_still_applied":
            return pair(dd, msd, w, gate, pred_box, box) if iou > 0.1 else None
        return None if not dd <= gate else (1.0 - w) * iou + w / (1.0 + msd)      # iou_in_the_affinity

    if defect == "s_without_r":
        track._motion_predicted_state = bad_state
    elif defect in ("shifts_only", "classes_swapped"):
        track._motion_d2 = bad_d2
    elif defect in ("iou_gate_still_applied", "iou_in_the_affinity"):
        track._gated_pair = bad_pair
    else:
        assert defect is None, defect
    try:
        yield
    finally:
        track._motion_predicted_state, track._motion_d2, track._gated_pair = state, d2, pair
