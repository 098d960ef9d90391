"""CPU tests of tests/readout_cases.py: every float64 reference against something independent, every float32 restatement inside its
share of the bound, the coverage of the case tables, and the planted defects (each must miss the bound by DEFECT_MARGIN)."""
import numpy as np
import pytest
import torch

import fold_cases as FC
import readout_cases as RC
from oracle import air_oracle as O

F32, F64 = np.float32, np.float64
IW_BASE = [n for n, c in RC.IW_ROWS.items() if not c["data"]]


# ---------------------------------------------------------------------------------------------------------------
# references against something independent
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IW_BASE)
def test_logweight_reference_against_torch_distributions_and_the_oracle(name):
    c, d, ref = RC.IW_ROWS[name], RC.iw_data(name), RC.iw_ref64(name)
    T, R = c["T"], c["R"]
    pr = [torch.tensor(float(F32(v)), dtype=torch.float64) for v in RC.IW_PRIORS[c["prior"]]]
    N = torch.distributions.Normal
    t64 = {k: torch.from_numpy(np.asarray(d[k], F64)) for k in ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale")}
    assert (ref["n"] == d["n"]).all()
    table = torch.from_numpy(d["table"] / (d["table"].sum() if c["norm"] else 1.0))
    rows = 0
    for r in range(R):
        n = int(d["n"][r])
        if not np.isfinite(ref["logw"][r]) or not np.isfinite(ref["logq"][r]):
            continue
        lq = N(t64["what_loc"][:n, r], t64["what_scale"][:n, r]).log_prob(t64["what"][:n, r]).sum() + \
            N(t64["where_loc"][:n, r], t64["where_scale"][:n, r]).log_prob(t64["where"][:n, r]).sum()
        shift_loc = t64["where_loc"][:n, r, 1::2] if bool(torch.isnan(pr[4])) else pr[4].expand(n, 2)
        lp = N(pr[0], pr[1]).log_prob(t64["what"][:n, r]).sum() + N(pr[2], pr[3]).log_prob(t64["where"][:n, r, 0::2]).sum() + \
            N(shift_loc, pr[5]).log_prob(t64["where"][:n, r, 1::2]).sum()
        log_prior = O.num_steps_log_prob(table[None, :], torch.tensor([n]))[0]
        logw = -float(d["rec"][r]) + float(log_prior) - float(d["logp"][r]) + float(lp - lq)
        assert abs(logw - ref["logw"][r]) <= 1e-11 * ref["S_logw"][r], (name, r)
        assert abs(float(lq) + float(d["logp"][r]) - ref["logq"][r]) <= 1e-11 * ref["S_logq"][r], (name, r)
        rows += 1
    assert rows >= 1


def test_logweight_planted_rows_have_the_class_of_the_plain_formula():
    ref, d = RC.iw_ref64("Iw_32x9x3x8"), RC.iw_data("Iw_32x9x3x8")
    assert d["n"][:4].tolist() == [32, 0, 1, 31]
    assert RC.classes(ref["logw"]).tolist() == [0, 0, 0, 0, 3, 3, 0, 2, 1]          # scale 0 (x != loc, x == loc), big z, prior 0, logp -inf
    assert RC.classes(ref["logq"]).tolist() == [0, 0, 0, 0, 3, 3, 0, 0, 2]
    d = RC.iw_data("Iw_3x7x1x50")
    assert d["n"][2:5].tolist() == [1, 1, 0] and d["presence"][:, 2].tolist() == [1.0, 0.5, 1.0] and d["presence"][:, 3].tolist() == [1.0, 0.0, 1.0]
    for k in ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale"):
        assert np.isnan(d[k][1:, 2]).all() and np.isnan(d[k][:, 4]).all()


@pytest.mark.parametrize("name", list(RC.RED_CASES))
def test_reduce_reference_against_torch(name):
    c, d = RC.RED_CASES[name], RC.red_data(name)
    ref = RC.red_ref64(d["logw"], d["n"], c["T"])
    lw = torch.from_numpy(d["logw"].astype(F64))
    assert np.allclose(ref["iw_bound"], (torch.logsumexp(lw, 1) - np.log(c["K"])).numpy(), rtol=1e-12, atol=0)
    sm = torch.softmax(lw, 1)
    assert np.allclose(ref["ess"], (1.0 / (sm * sm).sum(1)).numpy(), rtol=1e-10)
    n = torch.from_numpy(d["n"].astype(np.int64))
    for cc in range(c["T"] + 1):
        assert np.allclose(ref["q_n"][:, cc], torch.where(n == cc, sm, torch.zeros_like(sm)).sum(1).numpy(), rtol=1e-10, atol=1e-300)
    outside = ((d["n"] < 0) | (d["n"] > c["T"]))
    share = torch.where(torch.from_numpy(outside), sm, torch.zeros_like(sm)).sum(1).numpy()
    assert np.allclose(ref["q_n"].sum(1), 1.0 - share, rtol=1e-10, atol=1e-12)                # counts outside 0..T are counted nowhere
    if c["B"] >= 4 and c["K"] > 1:
        assert share[3] > 0.1


def test_reduce_nonfinite_table_is_what_the_restatement_gives():
    """the values RED_NONFINITE pins are what the kernel's order of operations gives in IEEE float32 (and what the docstring of
    iw_eval states)"""
    n = np.array([RC.RED_NONFINITE_COUNTS], np.int32)
    for name, (lw, iw, elbo, ess, q) in RC.RED_NONFINITE.items():
        r = RC.red_restate32(np.array([lw], F32), n, 2)
        for got, want in [(r["iw_bound"][0], iw), (r["elbo"][0], elbo), (r["ess"][0], ess)] + list(zip(r["q_n"][0], q)):
            assert np.isnan(got) if want == "nan" else got == want, (name, got, want)


def test_accumulate_restatement_and_tie_rule():
    rng = np.random.default_rng(3)
    B, T = 1000, 3
    q = rng.uniform(size=(B, T + 1)).astype(F32)
    q[5] = [0.25, 0.5, 0.5, 0.0]
    gt = RC.argmax_counts(q).astype(np.int32)
    assert gt[5] == 1 and RC.argmax_counts(q, tie_to_larger=True)[5] == 2
    v = [rng.standard_normal(B).astype(F32) * 3000 for _ in range(3)]
    acc = RC.accumulate64(*v, q, gt, [1.5, -2.5, 3.25, 7.0, 11.0])
    assert acc[3] == 7.0 + B and acc[4] == 11.0 + B
    for i in range(3):
        assert abs(acc[i] - ([1.5, -2.5, 3.25][i] + v[i].astype(F64).sum())) <= 1e-9
    assert RC.accumulate64(*v, q, None, [0, 0, 0, 7.0, 0])[3] == 7.0


@pytest.mark.parametrize("name", list(RC.SPREAD_CASES))
def test_spread_reference_against_torch(name):
    c, d = RC.SPREAD_CASES[name], RC.spread_data(name)
    T, B, K = c["T"], c["B"], c["K"]
    ref = RC.spread_ref64(d["logw"], d["n"], d["where"], T)
    sm = torch.softmax(torch.from_numpy(d["logw"].astype(F64)), 1)
    x = torch.from_numpy(d["where"].astype(F64)).reshape(T, B, K, 4)
    for t in range(T):
        wt = sm * torch.from_numpy(d["n"] > t)
        W = wt.sum(1)
        ok = (W > 0).numpy()
        assert np.allclose(ref["presence_iw"][t], W.numpy(), rtol=1e-10, atol=1e-300)
        mean = (wt[:, :, None] * x[t]).sum(1) / W[:, None]
        assert np.allclose(ref["mean"][t][ok], mean.numpy()[ok], rtol=1e-9)
        var = (wt[:, :, None] * (x[t] - mean[:, None, :]) ** 2).sum(1) / W[:, None]
        assert np.allclose(ref["std"][t][ok], var.sqrt().numpy()[ok], rtol=1e-6, atol=1e-14 * float(x.abs().max()))       # (equal values at 1e4: the mean's last place)
        assert np.isnan(ref["mean"][t][~ok]).all() and (ref["presence_iw"][t][~ok] == 0).all()
    for b, p in d["planted"].items():
        assert (ref["std"][p["single"], b] == 0).all() and np.isnan(ref["std"][p["empty"], b]).all()
        assert (ref["mean"][p["single"], b].astype(F32) == d["where"].reshape(T, B, K, 4)[p["single"], b, p["lone"]]).all()
        assert d["logw"][b, p["lone"]] < d["logw"][b].max()                                 # its weight is not exactly 1


def test_spread_presence_is_the_tail_sum_of_the_reduce_posterior():
    c, d = RC.SPREAD_CASES["Spr_K65_B5_T32"], RC.spread_data("Spr_K65_B5_T32")
    ref = RC.spread_ref64(d["logw"], d["n"], d["where"], c["T"])
    red = RC.red_ref64(d["logw"], d["n"], c["T"])
    for t in range(c["T"]):
        assert np.allclose(ref["presence_iw"][t], red["q_n"][:, t + 1:].sum(1), rtol=1e-10, atol=1e-15)


def test_select_reference_rules():
    lw = np.full((4, 80), -5.0, F32)
    lq = np.zeros((4, 80), F32)
    n = (np.arange(320).reshape(4, 80) % 7).astype(np.int32)
    lw[0, 5] = lw[0, 69] = 1.0                      # the same lane across the stride
    lw[1, 70] = lw[1, 5] = 2.0                      # different lanes
    lw[2, 3], lq[2, 3] = np.inf, -np.inf            # NaN score under criterion 1: skipped
    lw[2, 9] = -np.inf
    lw[3] = np.nan
    best, score, num, deg = RC.select_ref(lw, lq, n, 1)
    assert best.tolist() == [5, 5, 0, 0] and deg.tolist() == [0, 0, 0, 1]
    assert score.view(np.uint32)[3] == RC.QNAN_BITS and num[3] == n[3, 0]
    best0 = RC.select_ref(lw, lq, n, 0)[0]
    assert best0[2] == 3                            # +inf is a value under criterion 0


def test_count_inversion_boundaries_and_the_oracle_prior():
    assert RC.count_by_inversion(RC.DYADIC_TABLE, RC.DYADIC_U, 3).tolist() == RC.DYADIC_N
    table = O.geometric_prior(0.3, 5).numpy()
    u = np.random.default_rng(1).uniform(size=2000).astype(F32)
    n = RC.count_by_inversion(table, u, 5)
    cum = np.cumsum(table[:5]) / table.sum()
    assert (n == (cum[None, :] <= u.astype(F64)[:, None]).sum(1)).mean() > 0.999            # (u * total against cum / total: a last place)
    freq = np.bincount(n, minlength=6) / 2000.0
    assert np.abs(freq - table / table.sum()).max() < 0.04


def test_latents_reference_guard_and_clip():
    d = RC.gen_data("Gn_3x5x52")
    n = np.clip(d["n_in"], 0, 3)
    ref = RC.latents_ref64(d, 3, RC.GEN_GUARD, n)
    g = float(F32(RC.GEN_GUARD))
    assert ref["where"][0, 1, 0] == g and ref["where"][0, 2, 2] == -g and 0 < ref["where"][0, 3, 1] < g
    assert ref["guarded"].sum() == 2
    assert ref["presence"].sum(0).tolist() == n.tolist()
    assert d["n_in"].min() < 0 and d["n_in"].max() > 3


def test_observe_reference_normals_and_clamps():
    z = FC.noise_ref(RC.OBS_SEED, RC.OBS_OFFSET + 7, 12, 0)[0].numpy()
    z0 = FC.noise_ref(RC.OBS_SEED, RC.OBS_OFFSET, 40, 0)[0].numpy()
    assert (z == z0[28:40]).all()                                                         # counter_base 7: seven quads further on
    canvas = np.array([0.5, np.nan, -3.0, 9.0], F32)
    mean, obs, bnd = RC.observe_ref(canvas, 2.0, 0.0, 0, -1.0, 4.0, noise=False)
    assert obs.tolist() == [1.0, -1.0, -1.0, 4.0] and (bnd == 0).all()                     # a NaN pixel under a finite lo: lo
    _, obs, _ = RC.observe_ref(canvas, 2.0, 0.0, 0, RC.NAN, 4.0, noise=False)
    assert obs[1] == 4.0 and obs[2] == -6.0                                                # lo NaN: no lower clamp; fminf drops the NaN too
    _, obs, _ = RC.observe_ref(canvas, 2.0, 0.0, 0, RC.NAN, RC.NAN, noise=False)
    assert np.isnan(obs[1]) and obs[3] == 18.0


# ---------------------------------------------------------------------------------------------------------------
# the restatements' share of every bound
# ---------------------------------------------------------------------------------------------------------------
def _measured():
    w = {}

    def note(k, v):
        w[k] = max(w.get(k, 0.0), v)

    for name, c in RC.IW_ROWS.items():
        ref = RC.iw_ref64(name)
        for V in sorted({1, c["V"]}):
            lw, lq = RC.iw_restate32(name, V)
            note("logw", RC.worst_ratio(lw, ref["logw"], ref["S_logw"]))
            note("logq", RC.worst_ratio(lq, ref["logq"], ref["S_logq"]))
    for name, c in RC.RED_CASES.items():
        d = RC.red_data(name)
        ref, r32 = RC.red_ref64(d["logw"], d["n"], c["T"]), RC.red_restate32(d["logw"], d["n"], c["T"])
        for k in ("iw_bound", "elbo", "ess", "q_n"):
            note(k, RC.worst_ratio(r32[k], ref[k], ref["S_" + k]))
    for name, c in RC.GEN_ROWS.items():
        d = RC.gen_data(name)
        ref = RC.latents_ref64(d, c["T"], 0.0, np.zeros(c["R"], np.int32))
        wh, we = RC.latents_restate32(d)
        note("latents", RC.worst_ratio(wh, ref["what"], ref["S_what"]))
        note("latents", RC.worst_ratio(we, ref["where"], ref["S_where"]))
    for name, c in RC.SPREAD_CASES.items():
        d = RC.spread_data(name)
        ref = RC.spread_ref64(d["logw"], d["n"], d["where"], c["T"])
        res = RC.spread_ref64(d["logw"], d["n"], d["where"], c["T"], lanes=True)
        for k in ("mean", "std", "presence_iw"):
            assert (RC.classes(ref[k]) == RC.classes(res[k])).all()
            fin = np.isfinite(ref[k])
            den, err = 2.0 ** -53 * ref["S_" + k][fin], np.abs(ref[k][fin] - res[k][fin])
            assert (err[den == 0] == 0).all()
            if (den > 0).any():
                note("spread64", float((err[den > 0] / den[den > 0]).max()))
    return w


def test_restatements_keep_their_share():
    w = _measured()
    print("\n  worst restatement error / (2^-24 S):", {k: round(v, 3) for k, v in w.items()})
    for k, const in RC.CONST.items():
        assert w[k] <= RC.RESTATEMENT_SHARE * const, (k, w[k], const)
        assert w[k] <= RC.RESTATEMENT_RATIO[k] * 1.001 and const == np.ceil(4 * RC.RESTATEMENT_RATIO[k]), (k, w[k])
    assert w["spread64"] <= RC.RESTATEMENT_SHARE * RC.SPREAD_F64_CONST and w["spread64"] <= RC.SPREAD_F64_RATIO * 1.001
    assert RC.SPREAD_F64_CONST == np.ceil(4 * RC.SPREAD_F64_RATIO)


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_named_by_a_row():
    missing = set(RC.INSTANTIATIONS) - RC.named_instantiations()
    assert not missing, missing
    assert {c["V"] for n, c in RC.IW_ROWS.items() if c["off"]} == {1, 2}                   # V = 1 and V = 2 by alignment
    assert RC.IW_ROWS["Iw_3x5x1x6"]["V"] == 2 and RC.IW_ROWS["Iw_3x7x1x50"]["V"] == 2 and RC.IW_ROWS["Iw_5x6x3x12"]["V"] == 4
    assert {c["K"] for c in RC.RED_CASES.values()} == {1, 2, 63, 64, 65, 200, 4099}
    assert {c["B"] for c in RC.RED_CASES.values()} == {1, 5, 257} and {c["T"] for c in RC.RED_CASES.values()} == {1, 3, 32}
    assert {c["K"] for c in RC.SPREAD_CASES.values()} == {1, 5, 64, 65, 200}
    assert {c["B"] for c in RC.SPREAD_CASES.values()} == {1, 5} and {c["T"] for c in RC.SPREAD_CASES.values()} == {1, 3, 32}
    assert {c["V"] for n, c in RC.GEN_ROWS.items() if c["off"]} == {1, 2}


# ---------------------------------------------------------------------------------------------------------------
# planted defects: DESIGN.md's criterion -- a defect of known size misses at every touched element, one of random size at the median
# ---------------------------------------------------------------------------------------------------------------
def _margins(bad, ref, bnd, keep=None):
    """error / bound at the touched elements (those the defect moves at all); a finite value turned non-finite counts as infinite.
    keep: the elements whose bound the case did not inflate on purpose (a known-size defect must miss at every one of THOSE, and they
    must be a quarter of the finite elements at least: the GEMM group's criterion)"""
    bad, ref, bnd = (np.asarray(a, F64).reshape(-1) for a in (bad, ref, bnd))
    fin = np.isfinite(ref)
    if keep is not None:
        assert 4 * int((fin & keep).sum()) >= int(fin.sum())
        fin = fin & keep
    with np.errstate(all="ignore"):
        ratio = np.where(np.isfinite(bad[fin]), np.abs(bad[fin] - ref[fin]) / bnd[fin], np.inf)
    return ratio[ratio > 0]


@pytest.mark.parametrize("defect,known", [("step_n_included", True), ("step_before_n_dropped", False), ("shift_not_centred", False),
                                          ("log_p_scale_dropped", True), ("table_not_normalised", True)])
def test_planted_defects_of_the_log_weight(defect, known):
    worst = np.inf
    for name in IW_BASE:
        c = RC.IW_ROWS[name]
        if (defect == "shift_not_centred" and c["prior"] != "centred") or (defect == "table_not_normalised" and not c["norm"]):
            continue
        ref, bad = RC.iw_ref64(name), RC.iw_ref64(name, defect)
        keep = np.array([c["rows"].get(r) != "bigz" for r in range(c["R"])])                # z * z up to 1e8 in S: the bound is 1e4 times wider there
        m = _margins(bad["logw"], ref["logw"], RC.bound("logw", ref["S_logw"]), keep if known else None)
        if len(m) == 0:
            continue
        if defect == "step_n_included":
            assert np.isinf(m).all()                                                      # every row behind n is NaN: a mask error is a NaN
        worst = min(worst, float(m.min() if known else np.median(m)))
    print(f"\n  {defect}: margin {worst:.3g}")
    assert worst >= RC.DEFECT_MARGIN


def test_planted_defects_of_the_reduce():
    d = RC.red_data("Red_K65_B257_T32")
    ref = RC.red_ref64(d["logw"], d["n"], 32)
    bad = RC.red_ref64(d["logw"], d["n"], 32, "no_shift")
    assert np.isneginf(bad["iw_bound"]).all() and np.isfinite(ref["iw_bound"]).all()         # exp(-3000) is 0: the shift matters here
    bad = RC.red_ref64(d["logw"], d["n"], 32, "ess_s1_over_s2")
    keep = np.array([RC.RED_KINDS[b % 5] in ("equal", "outside", "narrow") for b in range(257)])    # (one dominant particle: s1 = s2 = 1)
    m = _margins(bad["ess"], ref["ess"], RC.bound("ess", ref["S_ess"]), keep)
    assert len(m) >= 150 and m.min() >= RC.DEFECT_MARGIN, m.min()
    d = RC.red_data("Red_K2_B257_T1")
    q = RC.red_restate32(d["logw"], d["n"], 1)["q_n"]
    ties = q[:, 0] == q[:, 1]
    assert ties.sum() >= 50                                                                # the all-equal images: q_n[0] == q_n[T] == 0.5
    assert (RC.argmax_counts(q)[ties] == 0).all() and (RC.argmax_counts(q, tie_to_larger=True)[ties] == 1).all()


def test_planted_defects_of_the_spread_and_the_inversion():
    c, d = RC.SPREAD_CASES["Spr_K65_B5_T32"], RC.spread_data("Spr_K65_B5_T32")
    ref = RC.spread_ref64(d["logw"], d["n"], d["where"], c["T"])
    bad = RC.spread_ref64(d["logw"], d["n"], d["where"], c["T"], "has_step_ge")
    m = _margins(bad["presence_iw"], ref["presence_iw"], RC.spread_bound(ref["presence_iw"], ref["S_presence_iw"]))
    assert len(m) > 50 and np.median(m) >= RC.DEFECT_MARGIN
    m = _margins(bad["mean"], ref["mean"], RC.spread_bound(ref["mean"], ref["S_mean"]))
    assert np.median(m) >= RC.DEFECT_MARGIN
    bad = RC.spread_ref64(d["logw"], d["n"], d["where"], c["T"], "no_single_rule", lanes=True)
    p = d["planted"][1]
    assert (bad["std"][p["single"], 1] != 0).any()                                         # (w x) / w is not x: the rule is needed
    strict = RC.count_by_inversion(RC.DYADIC_TABLE, RC.DYADIC_U, 3, strict=True)
    assert (strict != np.array(RC.DYADIC_N))[1:3].all() and (strict == np.array(RC.DYADIC_N))[3:].all()


# ---------------------------------------------------------------------------------------------------------------
# Ps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Ps_3x9x8", "Ps_32x9x4", "Ps_1x1x1"])
def test_count_chain_against_the_oracle(name):
    d = RC.ps_data(name)
    n_hat, q, score = RC.count_chain64(d["prob"])
    ok = ~np.isnan(d["prob"]).any(0)
    p = torch.from_numpy(d["prob"].astype(F64).T[ok].copy())
    ref = O.bernoulli_to_modified_geometric(p).numpy()
    assert np.allclose(q[ok], ref, rtol=1e-12, atol=1e-300)
    assert (q[ok][np.arange(ok.sum()), n_hat[ok]] == q[ok].max(1)).all()
    first = np.array([int(np.flatnonzero(row == row.max())[0]) for row in q[ok]])
    assert (n_hat[ok] == first).all()                                                      # ties go to the smaller count
    assert np.allclose(score[:, ok], np.stack([ref[:, t + 1:].sum(1) for t in range(d["prob"].shape[0])]), rtol=1e-12, atol=1e-300)


def test_boxes_and_the_scan_defect():
    from attend_infer_repeat_amd.evaluation import attention_box
    box, S = RC.boxes64(np.array([[0.5, 0.25, -0.5, 0.0]], F32), 20, 10)
    assert box[0].tolist() == list(attention_box((0.5, 0.25, -0.5, 0.0), 10, 20)) == [3.75, 15.0, 5.0, -10.0]
    assert S[0].tolist() == [8.75, 15.0, 5.0, 10.0]
    for R in RC.PS_SCAN_R:
        n = np.full(R, 32)
        good, bad = RC.exclusive_scan(n), RC.exclusive_scan(n, carry=False)
        assert good[R] == 32 * R and (good[:-1] == 32 * np.arange(R)).all()
        assert (good != bad).any() == (R > 1024), R                                        # only a second pass shows the defect


# ---------------------------------------------------------------------------------------------------------------
# Ps: the render
# ---------------------------------------------------------------------------------------------------------------
def test_render_form_mirror_against_the_library_query():
    """the Python mirror of air_parse_render's form rule against air_parse_render_form over seeded random shapes (host only: the
    query reads shapes and addresses, nothing is dereferenced)"""
    import ctypes
    from attend_infer_repeat_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7)
    base = 1 << 24
    seen = set()
    for i in range(400):
        T, R = int(rng.integers(1, 33)), int(rng.choice([1, 2, 7, 100, 256, 257, 512, 513, 2048, 2049, 5000]))
        H, W, h, w = (int(rng.integers(1, 70)) for _ in range(4))
        bands, goff = int(rng.integers(1, 10)), int(rng.integers(0, 2))
        m = RC.render_form(T, R, H, W, h, w, bands, goff)
        f = _lib.AirWarpForm()
        p = ctypes.c_void_p
        st = lib.air_parse_render_form(p(base + 4 * goff), p(base), p(base), p(base), p(base), None, p(base), p(base), T, R, H, W, h, w, bands,
                                       ctypes.byref(f))
        if m["lds_bytes"] > RC.CV_MAX_LDS:
            assert st == -5
            continue
        assert st == 0
        got = f.as_dict()
        assert {k: got[k] for k in m if k != "rule"} == {k: v for k, v in m.items() if k != "rule"}, (T, R, H, W, h, w, bands, got, m)
        seen.add((m["rule"], m["resident_cap"], m["vec4_glimpse"]))
    assert {s[0] for s in seen} == {"px", "512", "st"} and {s[1] for s in seen} == {0, 1} and {s[2] for s in seen} == {0, 1}


def test_render_rows_reach_every_form():
    forms = {n: RC.render_form(c["T"], c["R"], c["H"], c["W"], c["h"], c["w"], c["bands"], c["off"].get("glimpse", 0))
             for n, c in RC.PR_ROWS.items()}
    assert {f["rule"] for f in forms.values()} == {"px", "512", "st"}
    assert {f["resident_cap"] for f in forms.values()} == {0, 1}
    assert {f["vec4_glimpse"] for f in forms.values()} == {0, 1}
    assert set().union(*[RC.pr_pack_ok(n) for n in RC.PR_ROWS]) == {True, False}
    assert forms["Pr_65x64"]["threads"] == 1024 and 65 * 64 > 4 * 1024                     # the second prefetch
    for n in RC.PR_ROWS:                                                                   # no row is empty: some image has a present step
        assert (RC.pr_ref64(n)["reconstruction"] != 0).any() and (RC.pr_data(n)["presence"] > 0.5).any(), n
    assert forms["Pr_21x19_odd_W"]["threads"] == 448 and forms["Pr_R300"]["threads"] == 512 and forms["Pr_R600"]["threads"] == 256
    assert RC.PR_ROWS["Pr_5x6"]["H"] * RC.PR_ROWS["Pr_5x6"]["W"] % 4 == 2                   # the last quad is cut by npx


@pytest.mark.parametrize("name", ["Pr_21x19_odd_W", "Pr_5x6", "Pr_T32"])
def test_render_reference_against_the_oracle_write(name):
    c, d, ref = RC.PR_ROWS[name], RC.pr_data(name), RC.pr_ref64(name)
    T, nref = c["T"], d["nref"]
    mult = float(F32(RC.PR_MULT))
    for t in range(T):
        out = O.st_write(torch.from_numpy(d["glimpse"][t, :nref].astype(F64)), torch.from_numpy(d["where"][t, :nref].astype(F64)),
                         (c["H"], c["W"])).numpy()
        want = mult * out * (d["presence"][t, :nref] > 0.5)[:, None, None]
        assert np.abs(ref["layers"][t] - want).max() <= 1e-9 * (1 + np.abs(want).max()), (name, t)
    assert np.allclose(ref["reconstruction"], ref["layers"].sum(0))


def test_planted_defects_of_the_owner_rule():
    rng = np.random.default_rng(9)
    T, R, H, W = 3, 2, 5, 6
    lay = rng.uniform(0.1, 1.0, (T, R, H, W)).astype(F32)
    lay[2] = lay[0]                                                                        # equal layers at steps 0 and 2
    lay[1] *= F32(0.05)
    pres = np.ones((T, R), F32)
    own, top = RC.owner_rule(lay, pres, 0.0)
    assert (own == 0).all() and (RC.owner_rule(lay, pres, 0.0, tie_to_larger=True)[0] == 2).all()
    thr = float(top[1, 2, 3])
    own_t = RC.owner_rule(lay, pres, thr)[0]
    assert own_t[1, 2, 3] == -1 and RC.owner_rule(lay, pres, thr, ge=True)[0][1, 2, 3] == 0
    lay[0, 0, 0, 0] = np.nan
    assert RC.owner_rule(lay, pres, 0.0)[0][0, 0, 0] == 2                                   # a NaN layer owns nothing
    pres[:, 1] = 0
    assert (RC.owner_rule(lay, pres, 0.0)[0][1] == -1).all()
