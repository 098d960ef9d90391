"""Host tests of the MOTS measures (attend_infer_repeat_amd/track.py: mots_contingency, reference_mots, mots_summary): the crafted
cases by hand, an independent brute force over pixel sets with rational IoUs on 300 seeded cases, the summary, the entry's prototype
and argument tuple, the refusals, and planted defects of the reference that the brute force catches."""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from track_mots_cases import CRAFTED, mots_case, planted_case, stack, table

from attend_infer_repeat_amd import _lib, track

ROOT = Path(__file__).resolve().parents[1]
RATES = ("motsa", "smotsa", "motsp", "recall", "precision", "mostly_tracked", "mostly_lost")


def reference(case):
    return track.reference_mots(table(case), case["n"], case["ids"], case["F"])


def summary(case):
    ref = reference(case)
    return track.mots_summary(ref["seq_mots_i"].sum(0), ref["seq_mots_f"].sum(0)), ref


# ---- 1. the crafted cases by hand ---------------------------------------------------------------------------------------------------------
def test_the_names_of_the_counters():
    assert track.MOTS_COUNTS == ("gt", "tp", "fn", "fp", "ids", "mostly_tracked", "mostly_lost", "gt_objects")
    assert track.MOTS_OUTPUTS == ("seq_mots_i", "seq_mots_f", "mots_match", "mots_iou")


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_case_counts(name):
    case = CRAFTED[name]
    ref = reference(case)
    got = dict(zip(track.MOTS_COUNTS, ref["seq_mots_i"][0].tolist()), soft=float(ref["seq_mots_f"][0]))
    assert got == case["want"], (name, got)
    assert ref["seq_mots_i"].dtype == np.int32 and ref["seq_mots_f"].dtype == np.float64
    assert ref["mots_match"].dtype == np.int32 and ref["mots_iou"].dtype == np.float32
    assert (ref["mots_match"] >= 0).sum() == got["tp"] and ((ref["mots_iou"] > 0) == (ref["mots_match"] >= 0)).all()


def test_crafted_case_figures():
    fig, _ = summary(CRAFTED["PERFECT"])
    assert fig["motsa"] == fig["smotsa"] == fig["motsp"] == fig["recall"] == fig["precision"] == 1.0 and fig["mostly_tracked"] == 1.0
    fig, _ = summary(CRAFTED["SPLIT"])
    assert fig["tp"] == 4 and fig["id_switches"] == 1 and fig["motsa"] == 0.75 and fig["smotsa"] == 0.75 and fig["motsp"] == 1.0
    fig, ref = summary(CRAFTED["EXACT_HALF"])
    assert fig["motsa"] == -1.0 and fig["smotsa"] == -1.0 and math.isnan(fig["motsp"]) and ref["mots_match"].tolist() == [[-1]]
    fig, ref = summary(CRAFTED["FIVE_EIGHTHS"])
    assert fig["soft"] == 0.625 and fig["motsa"] == 1.0 and fig["smotsa"] == 0.625 and fig["motsp"] == 0.625
    assert ref["mots_iou"].tolist() == [[0.625]] and ref["mots_match"].tolist() == [[0]]
    fig, ref = summary(CRAFTED["GAP"])
    assert fig["id_switches"] == 1 and ref["mots_match"][:, 0].tolist() == [0, -1, 0]
    fig, _ = summary(CRAFTED["UNCONFIRMED"])
    assert fig["misses"] == 1 and fig["false_positives"] == 0 and fig["motsa"] == 0.0
    fig, _ = summary(CRAFTED["SWAP"])
    assert fig["id_switches"] == 2 and fig["motsa"] == 0.75
    fig, ref = summary(CRAFTED["PERFECT"])
    assert ref["mots_match"].tolist() == [[0, 1], [0, 1], [1, 0], [0, 1]]          # the matched STEP; the ids did not switch
    fig, ref = summary(CRAFTED["NOTHING"])
    assert all(math.isnan(fig[k]) for k in RATES) and not ref["seq_mots_i"].any() and fig["gt"] == 0
    fig, ref = summary(CRAFTED["BIG"])
    assert fig["soft"] == 1.6e9 / 2.7e9 and ref["mots_iou"][0, 0] == np.float32(1.6e9 / 2.7e9) and fig["motsa"] == 1.0
    cont = CRAFTED["BIG"]["cont"].astype(np.int64)
    assert cont[0, 1].sum() > 2 ** 31 - 1 and 2 * cont[0, 1, 1] > 2 ** 31 - 1     # what the case is for


# ---- 2. the contingency table ---------------------------------------------------------------------------------------------------------------
def test_contingency_counts_pixels_and_drops_labels_out_of_range():
    case = mots_case(3, 2, 2, 3, seed=1, shape=(5, 7))
    cont = track.mots_contingency(case["owner"], case["gt"], 3, 2)
    assert cont.dtype == np.int32 and np.array_equal(cont, table(case)) and (cont.sum((1, 2)) == 35).all()
    four = track.mots_contingency(case["owner"].reshape(2, 3, 5, 7), case["gt"].reshape(2, 3, 5, 7), 3, 2)
    assert np.array_equal(four, cont)
    owner, gt = case["owner"].copy(), case["gt"].copy()
    owner[0, 0, 0], gt[0, 0, 1], owner[0, 0, 2], gt[0, 0, 3] = 3, 2, -2, -5        # a step past T - 1, a slot past G - 1, below -1
    dropped = track.mots_contingency(owner, gt, 3, 2)
    assert dropped[0].sum() == 31 and np.array_equal(dropped[1:], cont[1:]) and np.array_equal(dropped, table(dict(case, owner=owner, gt=gt)))
    with pytest.raises(ValueError, match="one shape"):
        track.mots_contingency(case["owner"], case["gt"][:, :4], 3, 2)
    with pytest.raises(ValueError, match="within 1"):
        track.mots_contingency(case["owner"], case["gt"], 3, 9)


# ---- 3. an independent brute force: pixel sets, rational IoUs ---------------------------------------------------------------------------
def brute_force(case):
    """MOTS of one case from its MAPS: pixel sets per step and per slot, IoU as a Fraction, ALL pairs with IoU > 1/2 -- asserted to be
    a one-to-one matching -- and the bookkeeping of the rule.  Returns the eight counters and soft as a Fraction, summed over the
    sequences."""
    T, G, F = case["T"], case["G"], case["F"]
    total = dict.fromkeys(track.MOTS_COUNTS, 0)
    soft = Fraction(0)
    for s in range(case["S"]):
        last, tracked, present = {}, [0] * G, [0] * G
        for f in range(F):
            r = s * F + f
            owner, gt = case["owner"][r].reshape(-1), case["gt"][r].reshape(-1)
            n = min(max(int(case["n"][r]), 0), T)
            hyp = {j: set(np.nonzero(owner == j)[0].tolist()) for j in range(n) if case["ids"][j, r] >= 0}
            hyp = {j: px for j, px in hyp.items() if px}
            slots = {g: set(np.nonzero(gt == g)[0].tolist()) for g in range(G)}
            slots = {g: px for g, px in slots.items() if px}
            pairs = [(g, j, Fraction(len(slots[g] & hyp[j]), len(slots[g] | hyp[j]))) for g in sorted(slots) for j in sorted(hyp)]
            pairs = [(g, j, iou) for g, j, iou in pairs if iou > Fraction(1, 2)]
            assert len({g for g, _, _ in pairs}) == len(pairs) == len({j for _, j, _ in pairs}), "IoU > 1/2 is no one-to-one matching"
            total["gt"] += len(slots)
            total["tp"] += len(pairs)
            total["fn"] += len(slots) - len(pairs)
            total["fp"] += len(hyp) - len(pairs)
            for g in slots:
                present[g] += 1
            for g, j, iou in pairs:
                soft += iou
                tracked[g] += 1
                i = int(case["ids"][j, r])
                total["ids"] += 1 if g in last and last[g] != i else 0
                last[g] = i
        for g in range(G):
            if present[g]:
                total["gt_objects"] += 1
                total["mostly_tracked"] += 1 if Fraction(tracked[g], present[g]) >= Fraction(4, 5) else 0
                total["mostly_lost"] += 1 if Fraction(tracked[g], present[g]) <= Fraction(1, 5) else 0
    return total, soft


def seeded(seed):
    rng = np.random.default_rng(10 ** 6 + seed)
    return mots_case(int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 3)), int(rng.integers(1, 5)), seed)


def compare(seed):
    case = seeded(seed)
    want, soft = brute_force(case)
    ref = track.reference_mots(track.mots_contingency(case["owner"], case["gt"], case["T"], case["G"]), case["n"], case["ids"], case["F"])
    got = dict(zip(track.MOTS_COUNTS, ref["seq_mots_i"].astype(np.int64).sum(0).tolist()))
    assert got == want, (seed, got, want)
    assert abs(Fraction(float(ref["seq_mots_f"].sum())) - soft) <= Fraction(1, 10 ** 12), seed
    return want


def test_reference_agrees_with_the_brute_force_on_300_seeded_cases():
    total = dict.fromkeys(track.MOTS_COUNTS, 0)
    for seed in range(300):
        for k, v in compare(seed).items():
            total[k] += v
    print("300 seeded cases: tp %d, fn %d, fp %d, ids %d" % (total["tp"], total["fn"], total["fp"], total["ids"]))
    assert total["tp"] > 0 and total["fn"] > 0 and total["fp"] > 0 and total["ids"] > 0, total


def test_planted_defects_of_the_reference_are_caught_by_the_brute_force(monkeypatch):
    def caught():
        for seed in range(300):
            try:
                compare(seed)
            except AssertionError:
                return True
        return False
    with monkeypatch.context() as m:                               # 1. >= in place of > at exactly 1/2
        m.setattr(track, "_mots_is_match", lambda inter, union: inter >= union - inter)
        assert caught()
        with pytest.raises(AssertionError):
            test_crafted_case_counts("EXACT_HALF")
    with monkeypatch.context() as m:                               # 2. the ground-truth area without the background's row
        m.setattr(track, "_mots_gt_area", lambda counts, g: sum(int(v) for v in counts[1:, g + 1]))
        assert caught()
    assert not caught()                                            # and the reference as it stands passes


def test_sequences_are_scored_on_their_own():
    a, b = mots_case(3, 2, 1, 4, seed=11), mots_case(3, 2, 1, 4, seed=12)
    both, ra, rb = reference(stack([a, b])), reference(a), reference(b)
    for k in ra:
        assert np.array_equal(both[k], np.concatenate([ra[k], rb[k]])), k
    planted = planted_case(5, 3, 2, 8, seed=3)
    assert reference(planted)["seq_mots_i"][:, 1].min() > 0        # the planted tables hold matches


# ---- 4. the summary, the prototype, the refusals -------------------------------------------------------------------------------------------
def test_summary_on_known_totals():
    fig = track.mots_summary([10, 8, 2, 1, 1, 1, 0, 2], 6.0)
    assert fig["motsa"] == 0.6 and fig["smotsa"] == 0.4 and fig["motsp"] == 0.75 and fig["recall"] == 0.8 and fig["precision"] == 8 / 9
    assert fig["mostly_tracked"] == 0.5 and fig["mostly_lost"] == 0.0 and fig["id_switches"] == 1 and fig["false_positives"] == 1
    assert fig["misses"] == 2 and fig["gt"] == 10 and fig["tp"] == 8 and fig["gt_objects"] == 2 and fig["soft"] == 6.0
    fig = track.mots_summary(np.zeros(8, np.int64), 0.0)
    assert all(math.isnan(fig[k]) for k in RATES)
    fig = track.mots_summary([4, 0, 4, 0, 0, 0, 1, 1], 0.0)        # ground truth and no hypothesis
    assert fig["motsa"] == 0.0 and fig["recall"] == 0.0 and math.isnan(fig["motsp"]) and math.isnan(fig["precision"])
    with pytest.raises(ValueError, match="mots_summary"):
        track.mots_summary([1, 2, 3], 0.0)


def test_header_prototype_ctypes_row_and_argument_tuple_agree():
    header = (ROOT / "include" / "air_hip.h").read_text()
    m = re.search(r"AIR_ENGINE_API int air_track_mots\(([^;]*?)\);", header, re.S)
    assert m, "air_track_mots is not declared in include/air_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const int *cont", "const int *num_objects", "const int *track_id", "int T", "int G", "int S", "int F", "int R",
                      "int *seq_mots_i", "double *seq_mots_f", "int *mots_match", "float *mots_iou", "void *stream"]
    names = tuple(p.replace("*", " ").split()[-1] for p in params)
    assert track.MOTS_ARGS == names[:-1] and names[-1] == "stream"  # (ENTRY_ARGS is held to its ten entries by an existing test)
    restype, argtypes = _lib.SIGNATURES["air_track_mots"]
    assert restype is _lib.c_int and len(argtypes) == len(params) == 13
    for p, t in zip(params, argtypes):
        assert (t is _lib.c_int) == ("*" not in p), p
    source = (ROOT / "attend_infer_repeat_amd" / "csrc" / "track_kernels.hip").read_text()
    m = re.search(r'extern "C" int air_track_mots\(([^)]*)\)', source)
    assert m and [" ".join(p.split()) for p in m.group(1).split(",")] == params
    assert "MOTS (air_track_mots" in track.__doc__ and "inter > union - inter" in track.__doc__ and "air_track_mots:" in header
    assert "search order cannot change the result" in " ".join(header.split())
    assert ", mask IoU," not in track.__doc__                      # no longer on the out-of-scope lists


def test_reference_refusals():
    c = mots_case(3, 2, 2, 4, seed=3)
    cont = table(c)
    with pytest.raises(ValueError, match="not sequences of"):
        track.reference_mots(cont, c["n"], c["ids"], 3)
    with pytest.raises(ValueError, match="ground-truth slots"):
        track.reference_mots(np.zeros((8, 4, 10), np.int32), c["n"], c["ids"], 4)
    with pytest.raises(ValueError, match="objects per frame"):
        track.reference_mots(np.zeros((1, 34, 2), np.int32), np.zeros(1), np.zeros((33, 1)), 1)
    with pytest.raises(ValueError, match="expected track_id"):
        track.reference_mots(cont, c["n"], c["ids"][:2], 4)
    with pytest.raises(ValueError, match="integer table"):
        track.reference_mots(cont.astype(np.float32), c["n"], c["ids"], 4)


def test_argument_refusals():
    from attend_infer_repeat_amd.mnist_model import AIRonMNIST
    from attend_infer_repeat_amd.scripts import multi_mnist
    with pytest.raises(ValueError, match="mots=True scores the tracks as masks"):
        AIRonMNIST.score_track(object(), None, None, mots=True)    # refused before anything of the model is touched
    assert not hasattr(track.StreamTracker, "mots") and not hasattr(track.StreamTracker, "mots_summary")
    assert hasattr(track.SequenceTracker, "mots") and hasattr(track.TrackStitcher, "mots")
    from attend_infer_repeat_amd.trajectory import TrajectorySmoother
    assert hasattr(TrajectorySmoother, "mots") and hasattr(TrajectorySmoother, "mots_summary")
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-mots", "--track-stream", "2"])
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-mots"])


def test_the_script_refuses_the_flag_on_a_stream_in_the_wording_of_the_other_refusals(capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-eval", "4", "--track-mots", "--track-stream", "2"])
    assert "--track-mots does not go with --track-stream (MOTS is out of scope on a stream)" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        multi_mnist.main(["--track-mots"])
    assert "--track-mots goes with --track-eval" in capsys.readouterr().err
