"""tests/edit_cases.py held on the CPU: the float64 references against the project's own (refine.reference_step, prune.reference_score,
prune.reference_select, propose.reference_residual, propose.reference_pool / reference_source) and against oracle.air_oracle.st_write,
the float32 restatements' share of every bound, the rows' promises (every kernel named, the big bands, the big carve) and the planted
defects.  No GPU."""
import numpy as np
import pytest
import torch

import edit_cases as EC
import readout_cases as RC
from attend_infer_repeat_amd import propose, prune, refine
from oracle import air_oracle as O

F32, F64 = np.float32, np.float64
RF_SMALL = ["Rf_1x1x1x1", "Rf_3x5x12x16", "Rf_3x5x6x9", "Rf_3x5x7x9"]
SC_SMALL = ["Sc_T2", "Sc_T4", "Sc_21x19_planted", "Sc_8x16", "Sc_5x6", "Sc_50x7"]


def _clean(d, keys):
    """the NaN rows behind n as zeros (the project's references multiply by a mask; NaN * 0 is NaN)"""
    return {k: (np.nan_to_num(v, nan=0.0) if k in keys else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------
# references against the project's
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RF_SMALL)
def test_refine_reference_against_the_project(name):
    c, d = EC.RF_ROWS[name], EC.rf_data(name)
    pr = EC.priors32(c["prior"])
    ad = EC.RF_ADAM
    ref = EC.rf_ref64(d, c, pr, 0)
    keys = ("what", "where", "where_loc", "dwhat", "dwhere") + EC.RF_UPDATED
    z = _clean(d, keys)
    c1, c2 = EC.bias_corrections(0)
    f = lambda k: float(F32(ad[k]))
    want = refine.reference_step(z["what"], z["where"], z["glimpse"], np.nan_to_num(d["presence"], nan=0.0), EC.f32_band_sum(d["rec_parts"])[None],
                                 z["dwhat"], z["dwhere"], z["where_loc"], pr, z["m_what"], z["v_what"], z["m_where"], z["v_where"],
                                 f("lr_what"), f("lr_where"), f("beta1"), f("beta2"), f("eps"), c1, c2, f("guard"), 0, 1)
    assert np.allclose(ref["J"], want["J"], rtol=1e-12, atol=1e-9)
    mask = ref["mask"][..., None]
    for base in ("what", "where"):
        for k, key in (("z", base), ("m", "m_" + base), ("v", "v_" + base)):
            got = np.where(mask, ref[base][k], 0.0)
            assert np.allclose(got, np.where(mask, want[key], 0.0), rtol=1e-12, atol=1e-12), (name, key)
    assert (want["take"]).all() and (EC.keep_rule(ref["J"], np.full(c["B"], np.nan), 0)).all()


def test_keep_rule_against_the_project():
    J = np.array([1.0, np.nan, -np.inf, np.inf, 2.0, 2.0, np.nan])
    best = np.array([1.0, 0.0, np.nan, 1e30, np.nextafter(2.0, 0), 3.0, np.nan])
    assert list(EC.keep_rule(J, best, 1)) == [False, False, True, True, True, False, False]
    assert EC.keep_rule(J, best, 0).all()                                        # iteration 0 takes whatever J is, a NaN included
    z = np.zeros((1, 7, 1))
    b0 = {"J": best, "iter": np.zeros(7, np.int64), "what": z, "where": np.zeros((1, 7, 4)), "glimpse": z}
    got = refine.reference_step(z, np.ones((1, 7, 4)), z, np.zeros((1, 7)), -J[None], None, None, np.zeros((1, 7, 4)),
                                (0.0, 1.0, 0.5, 0.5, 0.0, 1.0), None, None, None, None, 0.1, 0.1, 0.9, 0.999, 1e-8, 0.1, 0.001, 1e-3, 1, 0, best=b0)
    assert list(got["take"]) == list(EC.keep_rule(J, best, 1))


@pytest.mark.parametrize("name", ["Sel_3x5x12x16", "Sel_3x5x6x9", "Sel_6x4x8x4"])
@pytest.mark.parametrize("allc", [0, 1])
def test_select_reference_against_the_project(name, allc):
    c, d = EC.SEL_ROWS[name], EC.sel_data(name)
    pr = EC.priors32(c["prior"])
    J, S, n = EC.sel_ref64(d, c, pr, allc)
    want = prune.reference_select(d["what"], d["where"], d["glimpse"], d["score"], np.nan_to_num(d["presence"], nan=0.0), d["where_loc"], pr,
                                  d["prior"], c["norm"], allc, EC.f32_band_sum(d["rec_sub"]))
    assert (np.isnan(J) == np.isnan(want["J_sub"])).all() and (want["n"] == n).all()
    assert np.allclose(J, want["J_sub"], rtol=1e-12, atol=1e-9, equal_nan=True)
    for r in range(c["R"]):
        assert EC.visit(J[r], int(n[r]), c["T"], allc) == want["best_mask"][r]


@pytest.mark.parametrize("name", SC_SMALL)
def test_score_reference_against_the_project_and_the_oracle(name):
    c, d = EC.SC_ROWS[name], EC.sc_data(name)
    nref = d["nref"]
    layers, _ = EC.sc_layers64(name)
    for t in range(c["T"]):
        out = O.st_write(torch.from_numpy(d["glimpse"][t, :nref].astype(F64)), torch.from_numpy(d["where"][t, :nref].astype(F64)),
                         (c["H"], c["W"])).numpy()
        assert np.abs(layers[t] - out).max() <= 1e-9 * (1 + np.abs(out).max())
    for allc in (0, 1):
        ref, _ = EC.score_ref64(name, allc)
        want = prune.reference_score(d["glimpse"][:, :nref], d["where"][:, :nref], np.nan_to_num(d["presence"][:, :nref], nan=0.0),
                                     d["obs"][:nref], float(F32(EC.SC_MULT)), float(F32(EC.SC_STD)), allc, layers=layers)
        assert np.allclose(ref.sum(0), want, rtol=1e-11, equal_nan=True), (name, allc)
    own = prune.reference_score(d["glimpse"][:, :nref], d["where"][:, :nref], np.nan_to_num(d["presence"][:, :nref], nan=0.0), d["obs"][:nref],
                                float(F32(EC.SC_MULT)), float(F32(EC.SC_STD)), 1)
    assert np.allclose(EC.score_ref64(name, 1)[0].sum(0), own, rtol=1e-9)       # the project's own inverse warp


@pytest.mark.parametrize("name", ["Sc_21x19_planted", "Sc_8x16", "Sc_50x7"])
def test_residual_reference_against_the_project(name):
    d = EC.sc_data(name)
    nref = d["nref"]
    ref = EC.residual_ref64(name)
    res, energy = propose.reference_residual(d["glimpse"][:, :nref], d["where"][:, :nref], d["n"][:nref], d["obs"][:nref],
                                             float(F32(EC.RES_MULT)), float(F32(EC.RES_HI)))
    assert np.allclose(ref["res"], res, rtol=1e-9, atol=1e-12) and np.allclose(ref["parts"].sum(0), energy, rtol=1e-9)
    assert (ref["res"] > 0).any() and (ref["res"] == 0).any()


def test_residual_rule_clamps():
    obs, rec = np.array([0.9, 0.2, np.nan, 3.0, 0.5], F32), np.array([0.1, 0.5, 0.0, 0.5, np.nan], F32)
    assert list(EC.residual_rule(obs, rec, 1.0)) == [F32(0.9) - F32(0.1), 0.0, 0.0, 1.0, 0.0]
    assert EC.residual_rule(obs, rec, np.inf)[3] == 2.5 and EC.residual_rule(obs, rec, np.nan)[3] == 2.5     # a NaN bound clamps nothing


def test_pool_and_source_references():
    T, P, R, A, G = 3, 3, 5, 7, 9
    d = EC.pool_data(T, P, R, A, G)
    ref = propose.reference_pool(d["what"], d["where"], d["glimpse"], d["score"], d["counts"], d["prop_what"], d["prop_where"],
                                 d["prop_glimpse"], d["prop_score"], d["prior"], P, round=3, source_in=None)
    assert (ref["prior"][T + 1:] == 0).all() and len(ref["prior"]) == T + P + 1
    assert (ref["source"][T:] == (T + 3 * P + np.arange(P))[:, None]).all()
    assert ref["presence"].sum(0).tolist() == np.clip(d["counts"], 0, T).tolist()
    kept = np.array([[2, 0, 1, 5, 4, 3]] * R, np.int32).T
    assert (propose.reference_source(ref["source"], kept)[0] == ref["source"][2]).all()


# ---------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _ratio(out, ref, S):
    out, ref, S = (np.asarray(a, F64) for a in (out, ref, S))
    fin = np.isfinite(ref) & (S > 0)
    return float((np.abs(out[fin] - ref[fin]) / (RC.U * S[fin])).max()) if fin.any() else 0.0


def _measured():
    if _MEASURED:
        return _MEASURED
    w = {k: 0.0 for k in EC.CONST}
    note = lambda k, v: w.__setitem__(k, max(w[k], v))
    for name, c in EC.RF_ROWS.items():
        d, pr = EC.rf_data(name), EC.priors32(c["prior"])
        ref, got = EC.rf_ref64(d, c, pr, 0), EC.rf_restate32(d, c, pr, 0, c["V"])
        note("rf_J", _ratio(got["J"], ref["J"], ref["S_J"]))
        mask = ref["mask"][..., None]
        for base in ("what", "where"):
            for k, key in (("m", "m_" + base), ("v", "v_" + base), ("z", base)):
                r = ref[base]
                target = r["z_raw"] if (k, base) == ("z", "where") else r[k]
                sel = np.broadcast_to(mask, target.shape)
                note("rf_" + k, _ratio(got[key][sel], target[sel], r["S_" + k][sel]))
    for name, c in EC.SEL_ROWS.items():
        d, pr = EC.sel_data(name), EC.priors32(c["prior"])
        for allc in (0, 1):
            J, S, _ = EC.sel_ref64(d, c, pr, allc)
            note("sel_J", _ratio(EC.sel_restate32(d, c, pr, allc, c["V"]), J, S))
    for name, c in EC.SC_ROWS.items():
        ref, S = EC.score_ref64(name, 1)
        note("score", _ratio(EC.score_restate32(name, 1), ref, S))
    _MEASURED.update(w)
    return w


def test_restatements_keep_their_share():
    w = _measured()
    print("\n  worst restatement error / (2^-24 S):", {k: round(v, 3) for k, v in w.items()})
    for k, const in EC.CONST.items():
        assert w[k] <= EC.RESTATEMENT_SHARE * const, (k, w[k], const)
        assert w[k] <= EC.RESTATEMENT_RATIO[k] * 1.001 and const == np.ceil(4 * EC.RESTATEMENT_RATIO[k]), (k, w[k])


def test_restatement_visits_the_kernels_lane_order():
    """V changes the order of the adds and with it the float32 sum: the three restatements of one row differ somewhere"""
    c, d = EC.RF_ROWS["Rf_3x5x12x16"], EC.rf_data("Rf_3x5x12x16")
    pr = EC.priors32(c["prior"])
    J = [EC.rf_restate32(d, c, pr, 0, V)["J"] for V in (4, 2, 1)]
    assert not (J[0] == J[1]).all() or not (J[1] == J[2]).all()
    x = np.arange(1, 521, dtype=F32)
    assert EC.thread_sum32(x[None])[0] == x.sum() and EC.thread_sum32(x[None, :7])[0] == 28.0


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_named_by_a_row():
    assert len(EC.INSTANTIATIONS) == 3 + 6 + 3 + 3
    missing = set(EC.INSTANTIATIONS) - EC.named_instantiations()
    assert not missing, missing
    for rows in (EC.RF_ROWS, EC.SEL_ROWS):
        assert {c["V"] for c in rows.values() if "what" in c["off"]} == {1, 2}                      # V by alignment
        assert {c["V"] for c in rows.values() if not c["off"]} == {1, 2, 4}                         # V by A
    assert EC.vec_rule(12, 0) == 4 and EC.vec_rule(12, 1) == 1 and EC.vec_rule(12, 2) == 2 and EC.vec_rule(6, 0) == 2 and EC.vec_rule(7, 0) == 1
    assert {c["T"] for c in EC.SC_ROWS.values()} == {1, 2, 3, 4, 5, 6}


def test_band_mirror_and_the_big_rows():
    from attend_infer_repeat_amd import hip
    lib = None
    try:
        lib = hip.lib()
    except Exception:                                                                           # (no library without a build: the mirror stands alone)
        pass
    for R, H in [(1, 5), (1, 50), (2, 6), (2, 21), (3, 8), (129, 33), (129, 65), (128, 50), (256, 50), (300, 7)]:
        NB, RB = EC.unroll_bands(R, H)
        assert (NB - 1) * RB < H <= NB * RB
        if lib is not None:
            assert lib.air_canvas_unroll_bands(R, H) == NB, (R, H)
    assert EC.unroll_bands(1, 5) == (5, 1) and EC.unroll_bands(1, 50) == (8, 7) and EC.unroll_bands(129, 33) == (1, 33)
    px = {n: max((r1 - r0) * EC.SC_ROWS[n]["W"] for r0, r1 in EC.band_rows(EC.SC_ROWS[n])) for n in EC.SC_ROWS}
    assert px["Sc_33x32_one_band"] == 1056 > 1024 and px["Sc_65x32_one_band"] == 2080 > 2048
    assert max(v for k, v in px.items() if "one_band" not in k) <= 1024
    last = EC.band_rows(EC.SC_ROWS["Sc_50x7"])[-1]
    assert last == (49, 50)                                                                     # the short last band
    c = EC.SC_ROWS["Sc_51x51_glimpse"]
    NB, RB = EC.unroll_bands(c["R"], c["H"])
    for lds in (EC.score_lds_bytes(c["T"], RB, c["W"], c["h"], c["w"]), EC.residual_lds_bytes(c["T"], RB, c["W"], c["h"], c["w"])):
        assert 64 * 1024 < lds <= EC.CV_MAX_LDS, lds
    assert EC.score_lds_bytes(2, 1, 16, 150, 150) > EC.CV_MAX_LDS and EC.residual_lds_bytes(2, 1, 16, 150, 150) > EC.CV_MAX_LDS   # the refusals' shape
    for n, c2 in EC.SC_ROWS.items():
        if n != "Sc_51x51_glimpse":
            assert EC.score_lds_bytes(c2["T"], EC.unroll_bands(c2["R"], c2["H"])[1], c2["W"], c2["h"], c2["w"]) <= 64 * 1024


def test_presence_rows():
    assert [EC.presence_row(k, 3)[1] for k in EC.PRESENCE_KINDS] == [3, 0, 1, 1, 1]
    assert [EC.presence_row(k, 1)[1] for k in EC.PRESENCE_KINDS] == [1, 0, 1, 0, 0]
    d = EC.rf_data("Rf_3x5x12x16")
    assert d["n"].tolist() == [3, 0, 1, 1, 1] and np.isnan(d["what"][2, 1]).any() and np.isfinite(EC.rf_ref64(d, EC.RF_ROWS["Rf_3x5x12x16"],
                                                                                                    EC.priors32("centred"), 0)["J"]).all()
    assert (EC.rf_data("Rf_32x3x50x400")["n"] == 32).all()
    w = d["what"].view(np.uint32)
    assert (w[2, 1:, 0] == EC.PAYLOAD_BITS).all() and (w[2, 1:, -1] == 0x80000000).all()          # the payload NaN and -0.0 behind n


# ---------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------
def _margin(bad, ref, bnd):
    bad, ref, bnd = (np.asarray(a, F64).reshape(-1) for a in (bad, ref, bnd))
    fin = np.isfinite(ref) & (bad != ref)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(bad[fin]), np.abs(bad[fin] - ref[fin]) / bnd[fin], np.inf)


@pytest.mark.parametrize("defect,name", [("drop_past_1024", "Sc_33x32_one_band"), ("drop_past_1024", "Sc_65x32_one_band"),
                                         ("r0_last", "Sc_50x7"), ("no_cst", "Sc_8x16"), ("n_for_T", "Sc_8x16")])
def test_planted_defects_of_the_score(defect, name):
    ref, S = EC.score_ref64(name, 1)
    bad, _ = EC.score_ref64(name, 1, defect)
    if defect == "n_for_T":                                                                   # a rule defect: masks left unwritten
        assert (np.isnan(bad) & ~np.isnan(ref)).any()
        return
    m = _margin(bad, ref, RC.bound(EC.CONST["score"], S))
    assert len(m) and m.min() >= EC.DEFECT_MARGIN, (defect, name, m.min() if len(m) else None)


def test_planted_defects_of_the_select():
    d, c = EC.sel_planted_data(), EC.SEL_PLANTED_ROW
    pr = EC.priors32(c["prior"])
    J, S, n = EC.sel_ref64(d, c, pr, 1)
    P = EC.SEL_PLANTED
    got = {tag: EC.visit(J[r], int(n[r]), 3, 1) for r, tag in enumerate(P)}
    for tag, m in EC.SEL_PLANTED_MASKS.items():
        assert got[tag] == m, (tag, got[tag])
    r = P.index("twins_tie")
    assert J[r, 1] == J[r, 2] and np.nanmax(J[r]) == J[r, 1]
    assert EC.visit(J[r], 0, 3, 1, "tie_to_smaller") == 1
    r = P.index("start_ties")
    assert J[r, 1] == J[r, 2] and EC.visit(J[r], 1, 3, 1, "start_not_first") == 2
    r = P.index("start_nan")
    assert np.isnan(J[r, 7]) and got["start_nan"] != 7
    assert np.isneginf(J[P.index("plain"), [3, 5, 6]]).all()                                      # prior[2] = 0
    assert np.isposinf(J[P.index("one_pinf"), 4]) and np.isnan(J[P.index("all_nan")]).all()
    bad, _, _ = EC.sel_ref64(d, c, pr, 1, defect="prior_unnormalised")
    m = _margin(bad, J, RC.bound(EC.CONST["sel_J"], S))
    assert len(m) and m.min() >= EC.DEFECT_MARGIN


def test_planted_defects_of_the_refine_step():
    name = "Rf_3x5x12x16"
    c, d = EC.RF_ROWS[name], EC.rf_data(name)
    pr = EC.priors32(c["prior"])
    ref = EC.rf_ref64(d, c, pr, 0)
    mask = np.broadcast_to(ref["mask"][..., None], d["what"].shape)
    for defect, key in (("no_prior_term", "m"), ("no_bias_correction", "z")):
        bad = EC.rf_ref64(d, c, pr, 0, defect=defect)
        m = _margin(bad["what"][key][mask], ref["what"][key][mask], RC.bound(EC.CONST["rf_" + key], ref["what"]["S_" + key][mask]))
        assert len(m) and np.median(m) >= EC.DEFECT_MARGIN, (defect, np.median(m))
    J, best = np.array([1.0, 2.0]), np.array([1.0, np.nan])
    assert list(EC.keep_rule(J, best, 1)) == [False, True]
    assert list(EC.keep_rule(J, best, 1, "ge")) == [True, True] and list(EC.keep_rule(J, best, 1, "nan_best_stays")) == [False, False]


def test_planted_defects_of_the_residual():
    name = "Sc_12x9_kinds"
    ref = EC.residual_ref64(name)
    bad = EC.residual_ref64(name, defect="ones_counted")                                       # image 2 is (1, 0, 1): one leading one
    m = _margin(bad["res"], ref["res"], ref["bound"])
    assert len(m) and np.median(m) >= EC.DEFECT_MARGIN
    d = EC.sc_data(name)
    obs = d["obs"].copy()
    big = EC.residual_rule(F32(3.0) * obs, np.zeros_like(obs), EC.RES_HI)
    assert big.max() == 1.0 and EC.residual_rule(F32(3.0) * obs, np.zeros_like(obs), np.inf).max() > 1.0   # the clamp missing changes bits
