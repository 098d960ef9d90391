"""Host checks of tests/pointwise_cases.py (no GPU): every case builds; each reference agrees with an independent one (Ga: float64
autograd against fold_cases.gauss_head64 / gauss_dpre_by_hand where they apply, against the head written out by hand on every case,
against central differences for loc_mode 1 and the NaN-mean prior; Op: the float32 restatement against fold_cases.rmsprop64 within
fold_cases.RMS_TOL; Bf: the integer rounding against torch's CPU cast; Ut: the ordered column sum against float64); each float32
restatement of Ga stays within RESTATEMENT_SHARE of its bound (the worst ratios are printed: pytest -s); every planted defect misses
its bound by DEFECT_MARGIN, or differs in bits where the bar is bits, on at least one case; every strided case strides; every kernel
instantiation behind the entries is named by a case.

The planted defects.  Ga: the derivative of softplus taken at raw without the offset; the parity of the priors swapped; dsample2
dropped; the tanh derivative on the even dimensions; dkl_scale ignored; the NaN-mean term kept.  Op: the learning-rate boundary applied
per float4 at an unaligned n_model; the uncentred denominator; eps inside the square; a fused multiply-add in msi.  Bf: truncation; the
add-0x7fff-and-shift rounding without the NaN case."""
import os

import numpy as np
import pytest
import torch

import fold_cases as FC
import pointwise_cases as PC

F32 = np.float32
WORST = {}


def _ratio(kind, got, ref, S, what):
    got, ref, S = (np.asarray(t, np.float64) for t in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (what, got.shape, ref.shape, S.shape)
    err = np.abs(got - ref)
    assert (err[S == 0] == 0).all(), what
    r = float((np.maximum(err[S > 0] - PC.FLT_MIN, 0.0) / (PC.U32 * S[S > 0])).max()) if (S > 0).any() else 0.0
    if r > WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = (r, what)
    return r


# ---------------------------------------------------------------------------------------------------------------
# Ga
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.GA_RUN)
def test_ga_case_builds_and_the_two_float64_forms_agree(name):
    """autograd through the oracle's formulas against the head written out by hand (whose summands give S): forward and every
    backward option row of the case"""
    d, c = PC.ga_data(name), PC.GA[name]
    f = PC.ga_fwd_ref(name)
    for k in ("loc", "scale", "sample", "kl_row"):
        assert np.isfinite(f[k]).all(), (name, k)
        # (the oracle's softplus is the identity beyond 20, where log1p(exp(x)) is x + 2e-9: the switch rows differ by that)
        np.testing.assert_allclose(f["terms"][k], f[k], rtol=1e-8, atol=1e-300, err_msg=f"{name} {k}")
        assert (f["terms"]["S_" + k] >= 0).all()
    for opt in c["bwd"]:
        ref, S, hand = PC.ga_bwd_ref(name, opt)
        assert np.isfinite(ref).all() and ref.shape == (c["M"], 2 * c["D"])
        assert (np.abs(hand - ref) <= 0.05 * PC.U32 * S + 1e-300).all(), (name, opt, float(np.abs(hand - ref).max()))
    for kind, rows in d["planted"].items():
        assert rows, (name, kind)


def test_ga_references_against_the_fold_cases_forms():
    """fold_cases.gauss_head64 / gauss_dpre_by_hand (loc_mode 0, one prior, offset 0.5, dkl_scale 0.7) on a random head"""
    gen = torch.Generator().manual_seed(5)
    M, D = 9, 7
    pre, eps = torch.randn(M, 2 * D, generator=gen), torch.randn(M, D, generator=gen)
    ds, dkl = torch.randn(M, D, generator=gen), torch.randn(M, generator=gen)
    prior4 = FC.GB_PRIOR + FC.GB_PRIOR
    loc, scale, sample, kl = PC.gauss64(pre.double(), eps.double(), D, 0, FC.GB_OFFSET, prior4)
    s2, k2, l2, c2 = FC.gauss_head64(pre.double(), eps.double())
    for a, b in ((loc, l2), (scale, c2), (sample, s2), (kl, k2)):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-6, atol=1e-8)              # (the prior enters as float32 here, as a Python float there)
    mine = PC.gauss_bwd64(pre.numpy(), eps.numpy(), D, 0, FC.GB_OFFSET, prior4, ds.numpy(), None, dkl.numpy(), FC.GB_DKL_SCALE)
    np.testing.assert_allclose(mine, FC.gauss_dpre_by_hand(pre, eps, ds, dkl).numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(mine, FC.gauss_dpre64(pre, eps, ds, dkl).numpy(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name,opt", [("Ga_3x4_where", "ds_ds2"), ("Ga_13x8_where_planted", "scale07"), ("Ga_41x50_nan_mean", "ds_dkl"),
                                      ("Ga_5x65_where", "ds_ds2")])
def test_ga_backward_against_central_differences(name, opt):
    """loc_mode 1 and the NaN-mean prior: d/dpre of the scalar the backward differentiates, by central differences in float64"""
    d, c = PC.ga_data(name), PC.GA[name]
    kw = PC.ga_bwd_inputs(d, opt)
    D = c["D"]

    def scalar(p):
        _, _, sample, kl = PC.gauss64(torch.from_numpy(p), None if kw["eps"] is None else torch.from_numpy(kw["eps"]).double(), D,
                                      c["loc_mode"], c["offset"], c["prior4"], c["guard"])
        L = 0.0
        for k in ("dsample", "dsample2"):
            if kw[k] is not None:
                L = L + (sample * torch.from_numpy(kw[k]).double()).sum()
        if kw["dkl_row"] is not None:
            L = L + FC.f32v(kw["dkl_scale"]) * (torch.from_numpy(kw["dkl_row"]).double() * kl).sum()
        return float(L)

    ref, S, _ = PC.ga_bwd_ref(name, opt)
    p0 = d["pre"].astype(np.float64)
    rng = np.random.default_rng(0)
    # (not the three raw scales at 20 and its float32 neighbours: the oracle's softplus jumps by 2e-9 at 20, inside the difference's span)
    jump = {(r_, D + dd) for r_, dd in d["planted"].get("switch", [])[:3]}
    picks = [(r_, col) for r_, dd in sum(d["planted"].values(), []) for col in (dd, D + dd) if (r_, col) not in jump]
    picks += [(int(rng.integers(c["M"])), int(rng.integers(2 * D))) for _ in range(24)]
    picks = [p for p in picks if p not in jump]
    h = 1e-5
    for r_, col in picks:
        # a NaN prior mean follows the posterior's mean: the value of the scalar does not depend on it, and neither does its derivative
        up, dn = p0.copy(), p0.copy()
        up[r_, col] += h
        dn[r_, col] -= h
        num = (scalar(up) - scalar(dn)) / (2 * h)
        assert abs(num - ref[r_, col]) <= 1e-6 * (abs(ref[r_, col]) + S[r_, col]) + 1e-9, (name, r_, col, num, ref[r_, col])


def _ga_shares():
    for name in PC.GA_RUN:
        d, c = PC.ga_data(name), PC.GA[name]
        f = PC.ga_fwd_ref(name)
        loc, scale, sample, kl = PC.gauss_fwd32(d["pre"], d["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], c["guard"])
        if c["loc_mode"] == 0:
            assert PC.same_bits_or_nan(loc, d["pre"][:, :c["D"]]) == 0
        for kind, got in (("loc", loc), ("scale", scale), ("sample", sample), ("kl_row", kl)):
            _ratio(kind, got, f[kind], f["terms"]["S_" + kind], f"{kind} of {name}")
        for opt in c["bwd"]:
            kw = PC.ga_bwd_inputs(d, opt)
            ref, S, _ = PC.ga_bwd_ref(name, opt)
            got = PC.gauss_bwd32(d["pre"], kw["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], d["loc32"], d["scale32"],
                                 kw["dsample"], kw["dsample2"], kw["dkl_row"], kw["dkl_scale"], c["guard"])
            _ratio("dpre", got, ref, S, f"dpre of {name} [{opt}]")
        if c["kl_bwd"]:
            dl, dsc, S_l, S_s = PC.normal_kl_bwd64(d["loc32"], d["scale32"], c["prior4"], d["dkl_row"])
            gl, gs = PC.normal_kl_bwd32(d["loc32"], d["scale32"], c["prior4"], d["dkl_row"])
            _ratio("kl_bwd", gl, dl, S_l, f"dloc of normal_kl_bwd on {name}")
            _ratio("kl_bwd", gs, dsc, S_s, f"dscale of normal_kl_bwd on {name}")


def test_ga_restatement_share_of_every_bound():
    """the numpy float32 restatement of the kernels' formulas against the float64 references: the worst ratio of every kind of output is
    the one pointwise_cases.GA_RATIO records, and leaves RESTATEMENT_SHARE of the bound"""
    _ga_shares()
    for kind, const in PC.GA_CONST.items():
        worst, what = WORST[kind]
        print(f"\n[pointwise cases] Ga {kind}: worst restatement error / (2^-24 S) = {worst:.3f} ({what}); CONST {const}: share {worst / const:.3f}")
        assert worst / const <= PC.RESTATEMENT_SHARE, (kind, worst, what)
        assert abs(worst - PC.GA_RATIO[kind]) <= 0.01, (kind, worst, PC.GA_RATIO[kind])
        assert const == np.ceil(4 * PC.GA_RATIO[kind]), kind


def test_ga_switch_and_saturated_rows_are_what_they_claim():
    d = PC.ga_data("Ga_13x8_where_planted")
    c, D = d["case"], d["case"]["D"]
    raws = [float(F32(d["pre"][r_, D + dd] + F32(c["offset"]))) for r_, dd in d["planted"]["switch"]]
    assert raws == list(PC.SWITCH_TARGETS) and raws[0] < 20.0 == raws[1] < raws[2] < raws[3] == 30.0
    loc32 = d["loc32"]
    sat = [float(loc32[r_, dd]) for r_, dd in d["planted"]["saturated"]]
    assert sat[0] == 1.0 and sat[1] == 1.0 and sat[3] == -1.0 and 0.0 < sat[2] < 1e-12             # sigmoid(-30) is 9.4e-14, not 0
    got = PC.gauss_bwd32(d["pre"], d["eps"], D, 1, c["offset"], c["prior4"], loc32, d["scale32"], d["dsample"], None, d["dkl_row"], 1.0)
    for (r_, dd), zero in zip(d["planted"]["saturated"], (True, True, False, True)):
        assert (got[r_, dd] == 0.0) == zero, (r_, dd)                                                  # the derivative factor is exactly 0
    g = PC.ga_data("Ga_guard_where")
    f = PC.ga_fwd_ref("Ga_guard_where")
    vals = [float(f["sample"][r_, dd]) for r_, dd in g["planted"]["where_floor"]]
    G = FC.f32v(PC.GUARD)
    assert vals[:4] == [G, G, G, -G] and abs(vals[4] - G) < 1e-9 and abs(vals[5] - 1.5e-3) < 1e-9 and abs(vals[6] + 1.5e-3) < 1e-9
    r_, dd = g["planted"]["floored"][0]
    assert f["scale"][r_, dd] == G and PC.ga_bwd_ref("Ga_guard_where", "ds_dkl")[0][r_, g["case"]["D"] + dd] == 0.0


def test_ga_strided_cases_stride():
    for name in PC.GA_STRIDED_FWD:
        assert PC.GA[name]["M"] > PC.CAP_ROWS
    for name in PC.GA_STRIDED_BWD:
        assert PC.GA[name]["M"] * PC.GA[name]["D"] > PC.CAP_ITEMS
        assert -(-PC.GA[name]["D"] // 64) == 2                  # the lane loop runs twice as well
    for T, B in PC.HEADS_TB:
        assert T * B > PC.CAP_ROWS
    assert {T <= 8 for T, _ in PC.HEADS_TB} == {True, False}
    assert {PC.GA[n]["D"] for n in PC.GA} >= {1, 4, 50, 64, 65, 200}


@pytest.mark.parametrize("defect", PC.GA_DEFECTS)
def test_ga_planted_defect_misses_the_bound(defect):
    cases = {"dsp_no_offset": [("Ga_41x50", "ds_dkl")], "parity": [("Ga_41x50", "ds_dkl"), ("Ga_3x4_where", "ds_dkl")],
             "no_ds2": [("Ga_41x50", "ds_ds2"), ("Ga_3x4_where", "ds_ds2")], "tanh_even": [("Ga_3x4_where", "ds_dkl")],
             "no_dkl_scale": [("Ga_41x50", "scale07"), ("Ga_5x65_where", "scale07")], "nan_kept": [("Ga_41x50_nan_mean", "ds_dkl")]}[defect]
    best = 0.0
    for name, opt in cases:
        ref, S, _ = PC.ga_bwd_ref(name, opt)
        bad = PC.ga_defect(name, opt, defect)
        best = max(best, float((np.abs(bad - ref)[S > 0] / PC.ga_bound("dpre", S[S > 0])).max()))
    assert best >= PC.DEFECT_MARGIN, (defect, best)


# ---------------------------------------------------------------------------------------------------------------
# Op
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.OP))
def test_op_case_builds_and_the_restatement_is_the_float64_update(name):
    d = PC.op_data(name)
    c = d["case"]
    lo, hi = d["span"]
    assert 0 <= lo < hi <= c["n"] and 0 <= c["n_model"] <= c["n"]
    if c["entry"] == "rider":
        assert lo % 4 == 0 and hi % 4 == 0 and c["n_model"] % 4 == 0
    centred = c["entry"] != "rmsprop_plain"
    if c["state"] == "planted":
        share = float(np.isnan(d["ref32"]["p"][lo:hi]).mean())
        assert PC.NAN_SHARE[0] <= share <= PC.NAN_SHARE[1], (name, share)
        assert np.isfinite(d["ref32"]["ms"]).all() and np.isfinite(d["ref32"]["mg"]).all()
        assert (np.isnan(d["ref32"]["p"]) == np.isnan(d["ref32"]["mom"])).all()
        return
    ref = PC.op_ref64(d, centred)
    torch_ref = FC.rmsprop64(*(torch.from_numpy(d[k]) for k in PC.BUFS), torch.from_numpy(d["lr"]).double(), d["h"]["decay"],
                             d["h"]["momentum"], d["h"]["eps"], d["h"]["gscale"])
    for k, t in zip(("p", "ms", "mg", "mom"), torch_ref):
        if centred:
            np.testing.assert_allclose(ref[k], t.numpy(), rtol=1e-11, atol=1e-300)
        rtol, atol = FC.RMS_TOL[k]
        got = d["ref32"][k][lo:hi].astype(np.float64)
        assert np.isfinite(got).all()
        share = float((np.abs(got - ref[k][lo:hi]) / (atol + rtol * np.abs(ref[k][lo:hi]))).max())
        if share > WORST.get("Op", (0.0, ""))[0]:
            WORST["Op"] = (share, f"{k} of {name}")
        assert share <= PC.RESTATEMENT_SHARE, (name, k, share)


def test_op_restatement_share_of_rms_tol():
    """the float32 restatement against float64, as a share of fold_cases.RMS_TOL (the bar of the plain update on the device): printed"""
    for name in PC.OP:
        if PC.OP[name]["state"] != "planted":
            test_op_case_builds_and_the_restatement_is_the_float64_update(name)
    worst, what = WORST["Op"]
    print(f"\n[pointwise cases] Op: worst restatement error / RMS_TOL = {worst:.3f} ({what})")
    assert worst <= PC.RESTATEMENT_SHARE


@pytest.mark.parametrize("name", [n for n, c in PC.OP.items() if c["n"] >= 4099 and c["entry"] != "rmsprop_plain"])
def test_op_bit_bar_has_power_against_one_fused_multiply_add(name):
    """the restatement with the first product of msi fused into the sum differs in bits on at least 1 % of the elements of every case
    (of 4099 elements or more: a case of one to four elements cannot promise a share)"""
    d = PC.op_data(name)
    bad = PC.op_defect(name, "fma_msi")
    new = PC.rmsprop32(*(d[k] for k in PC.BUFS), d["lr"], d["h"])
    differ = PC.same_bits_or_nan(bad["ms"], new[1])
    assert differ >= 0.01 * d["case"]["n"], (name, differ)


@pytest.mark.parametrize("defect", PC.OP_DEFECTS)
def test_op_planted_defect_differs_in_bits(defect):
    names = {"per_float4": ["Op_epi_n4100_m6", "Op_epi_scalar_tail10"], "uncentred": ["Op_epi_vec_script"],
             "eps_in_square": ["Op_epi_vec_decay08", "Op_epi_planted_vec"], "fma_msi": ["Op_epi_vec_script"]}[defect]
    hit = 0
    for name in names:
        d = PC.op_data(name)
        bad = PC.op_defect(name, defect)
        n = sum(PC.same_bits_or_nan(bad[k], PC.rmsprop32(*(d[j] for j in PC.BUFS), d["lr"], d["h"])[i])
                for i, k in enumerate(("p", "ms", "mg", "mom")))
        if defect == "per_float4":
            c = d["case"]
            assert c["n_model"] % 4 != 0 and PC.epilogue_form(c["n"], c["n_model"]) == "scalar" and d["h"]["tail"] != 1.0
        hit += n
    assert hit > 0, defect


def test_op_strided_and_form_cases():
    for name in PC.OP_STRIDED:
        c = PC.OP[name]
        items = PC.epilogue_items(c["n"], c["n_model"], c["off"]) if c["entry"] == "epilogue" else c["n"]
        assert items > PC.CAP_ITEMS, name
    assert PC.epilogue_form(*[PC.OP["Op_epi_vec_strided"][k] for k in ("n", "n_model")]) == "vec"
    assert PC.epilogue_form(*[PC.OP["Op_epi_scalar_strided"][k] for k in ("n", "n_model")]) == "scalar"
    for b in PC.BUFS:
        c = PC.OP[f"Op_epi_off_{b}"]
        assert c["n"] % 4 == 0 and c["n_model"] % 4 == 0 and PC.epilogue_form(c["n"], c["n_model"], c["off"]) == "scalar"
    got = {(c["n"], c["n_model"]) for c in PC.OP.values() if c["entry"] == "epilogue"}
    for n in (1, 3, 4, 4099):
        assert {m for k, m in got if k == n} >= {m for m in (0, 4, n - 4, n) if 0 <= m <= n}, n
        assert any(m % 4 for k, m in got if k == n), n
    assert (PC.RNG0[1] + PC.RNG_INC) % 2 ** 64 == 2 ** 32 + 2 and PC.RNG_INC > 2 ** 32
    assert {c["hyper"] for c in PC.OP.values()} == set(PC.HYPER) and {c["counters"] for c in PC.OP.values()} == {"both", "no_gstep", "no_rng", "none"}


@pytest.mark.parametrize("name", list(PC.L2))
def test_l2_case_builds(name):
    d = PC.l2_data(name)
    c = d["case"]
    if name == "L2_32_ranges":
        assert len(c["ranges"]) == PC.L2_MAX_RANGES and any(lo % 4 for lo, _ in c["ranges"]) and not d["inside"].all()
    if name == "L2_strided":
        assert c["ranges"][0][0] == c["ranges"][0][1] and max(hi - lo for lo, hi in c["ranges"]) == PC.CAP_ITEMS + 5 > PC.CAP_ITEMS
    if c["status"] == 0:
        assert d["inside"].sum() == sum(hi - lo for lo, hi in c["ranges"])
        fused = (d["g"].astype(np.float64) + FC.f32v(PC.L2_WEIGHT) * d["p"].astype(np.float64)).astype(F32).astype(np.float64)
        assert (np.abs(fused - d["ref64"]) <= PC.L2_TOL[1] + PC.L2_TOL[0] * np.abs(d["ref64"])).all()


# ---------------------------------------------------------------------------------------------------------------
# Bf
# ---------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_against_the_cpu_cast():
    v = PC.bf16_values()
    assert len(v) % 4 == 0 and len(v) >= 4 * len(PC.CRAFTED) + 4099
    nan = PC.is_nan32(v)
    assert int(nan.sum()) == 4 * len(PC.NAN_PATTERNS) and {0x7F800001, 0x7FFFFFFF} <= set(PC.NAN_PATTERNS)
    t16 = torch.from_numpy(v.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (PC.bf16_rne(v)[~nan] == t16[~nan]).all()
    assert PC.is_nan16(t16[nan]).all() and PC.bf16_mismatches(v, t16) == 0
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81, 0x3FFF8000: 0x4000, 0x00000001: 0x0000,
            0x00008000: 0x0000, 0x00018000: 0x0002, 0x007FFFFF: 0x0080, 0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80, 0x7F7FFFFF: 0x7F80,
            0x80000000: 0x8000, 0xFF800000: 0xFF80}
    for k, h in want.items():
        assert int(PC.bf16_rne(np.array([k], np.uint32))[0]) == h, hex(k)


def test_bf16_planted_defects_differ():
    v = PC.bf16_values()
    assert PC.bf16_mismatches(v, PC.bf16_truncate(v)) >= 0.25 * 4099
    naive = PC.bf16_rne(v)                                              # the rounding applied to NaNs too
    assert int(PC.bf16_rne(np.array([0x7F800001], np.uint32))[0]) == 0x7F80 and int(PC.bf16_rne(np.array([0x7FFFFFFF], np.uint32))[0]) == 0x8000
    assert PC.bf16_mismatches(v, naive) >= 8                            # both patterns, in each of the four positions
    for name, c in PC.BF.items():
        n = len(PC.bf_source(name))
        assert (n % 4 == 0) == (c["tail"] == 0)
    assert PC.BF_STRIDED_N // 4 > PC.CAP_ITEMS


# ---------------------------------------------------------------------------------------------------------------
# Ut, coverage
# ---------------------------------------------------------------------------------------------------------------
def test_ut_references():
    assert max(PC.UT_SIZES) > PC.CAP_ITEMS and max(N for _, N in PC.COLSUM) > PC.CAP_ITEMS
    rng = np.random.default_rng(3)
    for M, N in PC.COLSUM[:3]:
        x = rng.standard_normal((M, N)).astype(F32)
        s = PC.colsum32(x)
        assert (np.abs(s - x.astype(np.float64).sum(0)) <= (M - 1) * PC.U32 * np.abs(x).astype(np.float64).sum(0)).all()
    for with_b in (False, True):
        a, b, alpha, beta = PC.axpby_inputs(257, with_b)
        ref = FC.f32v(alpha) * a.astype(np.float64) + (FC.f32v(beta) * b.astype(np.float64) if with_b else 0.0)
        unfused = (F32(alpha) * a + (F32(beta) * b if with_b else F32(0))).astype(F32)
        assert (np.abs(unfused - ref) <= PC.AXPBY_RTOL * np.abs(ref)).all()


def test_every_kernel_instantiation_is_named_by_a_case():
    named = PC.kernels_named()
    assert set(named) == set(PC.KERNELS)
    for k, cases in named.items():
        assert cases, f"no case launches {k}"
    src = ""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "attend_infer_repeat_amd", "csrc")
    for f in ("pointwise_kernels.hip", "engine_kernels.hip"):
        with open(os.path.join(root, f)) as fh:
            src += fh.read()
    for k in PC.KERNELS:
        assert f" {k.split('<')[0]}(" in src, k                        # the kernel still exists under this name
    for n in (1, 3, 4, 4099, PC.CAP_ITEMS + 3, 4 * PC.CAP_ITEMS + 4):
        assert f"Op_plain_n{n}" in PC.OP
    for n in (1, 3, 4, 4099, PC.CAP_ITEMS + 3):
        assert any(c["entry"] == "rmsprop" and c["n"] == n for c in PC.OP.values()), n
