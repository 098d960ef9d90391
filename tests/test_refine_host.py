"""Host-side tests of parse refinement (attend_infer_repeat_amd/refine.py): the argument checks, `reference_step` -- the numpy float64
restatement of air_refine_step -- on hand-derived cases, and the new entry in the header and in a library built here.  No GPU."""
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

from attend_infer_repeat_amd import refine
from attend_infer_repeat_amd.engine_config import EngineConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "air_hip.h")
PRIORS = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)


# ---- 1. check_arguments ---------------------------------------------------------------------------------------------------------
def test_check_arguments_accepts_the_scripts_configuration():
    cfg = EngineConfig(max_steps=3, explore_eps=1e-3, steps_pred_hidden=(128, 64), transform_var_bias=.5, step_bias=.75,
                       output_multiplier=.5)
    refine.check_arguments(cfg, 16, *refine.DEFAULT_LR)
    refine.check_arguments(cfg, 0, 0.0, 0.0)
    refine.check_arguments(dataclasses.replace(cfg, where_shift_prior=(None, 1.0)), 4, 1e-2, 1e-3, 0.0, 0.0, 1.0)


@pytest.mark.parametrize("kw,match", [
    (dict(steps=-1), "steps"), (dict(steps=1.5), "steps"),
    (dict(lr_what=-1e-3), "lr_what"), (dict(lr_where=-1e-3), "lr_where"), (dict(lr_what=float("nan")), "lr_what"),
    (dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta2=1.0), "beta2"), (dict(beta2=1.5), "beta2"),
    (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps")])
def test_check_arguments_refuses_bad_numbers(kw, match):
    args = dict(steps=4, lr_what=1e-2, lr_where=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        refine.check_arguments(EngineConfig(), **args)


@pytest.mark.parametrize("change,match", [
    (dict(what_prior=None), "what_prior"), (dict(where_scale_prior=None), "where_scale_prior"),
    (dict(where_shift_prior=None), "where_shift_prior"), (dict(discrete_steps=False), "discrete_steps"),
    (dict(mfma_dtype="bf16"), "bf16.*out of scope")])
def test_check_arguments_refuses_configurations(change, match):
    with pytest.raises(ValueError, match=match):
        refine.check_arguments(dataclasses.replace(EngineConfig(), **change), 4, 1e-2, 1e-2)


# ---- 2. reference_step on hand-derived cases ----------------------------------------------------------------------------------------
def _one_latent(z=0.5, d=0.25, lr=0.1, eps=1e-8, c=None, **kw):
    """T = B = A = 1, one present step; only what[0, 0, 0] has a gradient that matters"""
    a = lambda v, *s: np.full(s, v, np.float64)
    args = dict(what=a(z, 1, 1, 1), where=a(1.0, 1, 1, 4), glimpse=a(0.0, 1, 1, 2), presence=a(1.0, 1, 1), rec_parts=a(2.0, 2, 1),
                dwhat=a(d, 1, 1, 1), dwhere=a(0.0, 1, 1, 4), where_loc=a(0.0, 1, 1, 4), priors=PRIORS, m_what=a(0.0, 1, 1, 1),
                v_what=a(0.0, 1, 1, 1), m_where=a(0.0, 1, 1, 4), v_where=a(0.0, 1, 1, 4), lr_what=lr, lr_where=0.0, beta1=0.9,
                beta2=0.999, eps=eps, c1=1 - 0.9 if c is None else c[0], c2=1 - 0.999 if c is None else c[1], guard_eps=0.0, iter=0,
                do_update=1)
    args.update(kw)
    return refine.reference_step(**args)


def test_first_adam_step_is_lr_g_over_abs_g_plus_eps():
    for z, d in ((0.5, 0.25), (-2.0, 0.5), (0.0, -3.0)):
        g = d + z                                                  # prior N(0, 1): (z - 0) / 1
        out = _one_latent(z=z, d=d, lr=0.1, eps=1e-3)
        # m / c1 = g and sqrt(v / c2) = |g| after the first step, whatever the betas
        assert out["what"][0, 0, 0] == pytest.approx(z - 0.1 * g / (abs(g) + 1e-3), rel=1e-14)
        assert out["m_what"][0, 0, 0] == pytest.approx((1 - 0.9) * g, rel=1e-14)
        assert out["v_what"][0, 0, 0] == pytest.approx((1 - 0.999) * g * g, rel=1e-14)


def test_objective_has_the_half_log_two_pi_terms_and_adds_the_bands_in_order():
    out = _one_latent(z=0.5)
    # -rec + log N(0.5 | 0, 1) + 4 log N(1 | 0, 1)
    want = -(2.0 + 2.0) + (-0.125 - 0.5 * math.log(2 * math.pi)) + 4 * (-0.5 - 0.5 * math.log(2 * math.pi))
    assert out["J"][0] == pytest.approx(want, rel=1e-15)
    # a shift prior without loc is centred on where_loc: the shift terms lose their quadratic part when where == where_loc
    out = _one_latent(z=0.5, priors=(0.0, 1.0, 0.0, 1.0, None, 1.0), where_loc=np.ones((1, 1, 4)))
    assert out["J"][0] == pytest.approx(want + 2 * 0.5, rel=1e-15)
    # other prior scales: -log(scale) enters
    out = _one_latent(z=0.5, priors=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0))
    assert out["J"][0] == pytest.approx(want + 0.125 - 0.5 * 0.25 * 0.25 - math.log(2.0), rel=1e-15)


def test_keep_rule_rows():
    """iteration 0 takes even NaN; later: NaN never replaces, a tie keeps the earlier iteration, -inf is an ordinary value"""
    B = 6
    a = lambda v, *s: np.full(s, v, np.float64)
    base = dict(what=a(0.0, 1, B, 1), where=a(1.0, 1, B, 4), glimpse=a(0.0, 1, B, 2), presence=a(0.0, 1, B), dwhat=None, dwhere=None,
                where_loc=None, priors=PRIORS, m_what=None, v_what=None, m_where=None, v_where=None, lr_what=0.0, lr_where=0.0,
                beta1=0.9, beta2=0.999, eps=1e-8, c1=0.1, c2=0.001, guard_eps=0.0, do_update=0)
    # n = 0 everywhere: J = -rec.          image:   0     1      2       3       4        5
    rec0 = np.array([[np.nan, 5.0, 5.0, np.nan, np.inf, np.inf]])
    rec1 = np.array([[3.0, np.nan, 5.0, np.nan, np.inf, 7.0]])
    rec2 = np.array([[4.0, 4.0, 4.0, np.nan, 9.0, np.inf]])
    mark = lambda i: dict(what=a(float(i), 1, B, 1))
    s0 = refine.reference_step(**{**base, **mark(0)}, rec_parts=rec0, iter=0, best=None)
    assert s0["take"].all() and np.array_equal(s0["best"]["iter"], np.zeros(B))
    assert np.array_equal(np.isnan(s0["best"]["J"]), [True, False, False, True, False, False])
    s1 = refine.reference_step(**{**base, **mark(1)}, rec_parts=rec1, iter=1, best=s0["best"])
    #  finite replaces NaN | NaN never replaces | exact tie keeps the earlier | NaN after NaN | -inf == -inf: a tie | -7 > -inf
    assert s1["take"].tolist() == [True, False, False, False, False, True]
    s2 = refine.reference_step(**{**base, **mark(2)}, rec_parts=rec2, iter=2, best=s1["best"])
    #  -4 < -3 | -4 > -5 | -4 > -5 | NaN | -9 > -inf | -inf < -7
    assert s2["take"].tolist() == [False, True, True, False, True, False]
    assert s2["best"]["iter"].tolist() == [1, 2, 2, 0, 2, 1]
    assert s2["best"]["what"][0, :, 0].tolist() == [1.0, 2.0, 2.0, 0.0, 2.0, 1.0]          # the rows travel with the decision
    assert np.array_equal(s2["best"]["J"], [-3.0, -4.0, -4.0, np.nan, -9.0, -7.0], equal_nan=True)
    assert np.array_equal(s0["best"]["iter"], np.zeros(B))         # nothing was modified in place


def _random_case(seed, T=3, B=4, A=5, G=6, n=(0, 1, 2, 3)):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s)
    presence = (np.arange(T)[:, None] < np.array(n)[None, :]).astype(np.float64)
    return dict(what=r(T, B, A), where=r(T, B, 4), glimpse=r(T, B, G), presence=presence, rec_parts=np.abs(r(2, B)), dwhat=r(T, B, A),
                dwhere=r(T, B, 4), where_loc=r(T, B, 4), priors=(0.1, 1.5, 1.0, 0.5, None, 2.0), m_what=r(T, B, A),
                v_what=np.abs(r(T, B, A)), m_where=r(T, B, 4), v_where=np.abs(r(T, B, 4)), lr_what=1e-2, lr_where=1e-2, beta1=0.9,
                beta2=0.999, eps=1e-8, c1=0.19, c2=0.002, guard_eps=0.0, iter=1, do_update=1)


def test_absent_rows_are_untouched_and_present_rows_move():
    case = _random_case(3)
    out = refine.reference_step(**case)
    mask = case["presence"] > 0.5
    for k in ("what", "where", "m_what", "v_what", "m_where", "v_where"):
        assert np.array_equal(out[k][~mask], case[k][~mask]), k
        assert (out[k][mask] != case[k][mask]).all(), k
    for k in ("what", "where", "m_what", "presence"):               # the inputs themselves are left alone
        assert np.array_equal(case[k], _random_case(3)[k])
    # do_update = 0: nothing moves
    still = refine.reference_step(**{**case, "do_update": 0})
    for k in ("what", "where", "m_what", "v_what", "m_where", "v_where"):
        assert np.array_equal(still[k], case[k]), k


def test_learning_rate_zero_is_the_identity_on_its_group():
    case = _random_case(4)
    out = refine.reference_step(**{**case, "lr_what": 0.0, "guard_eps": 10.0})
    assert np.array_equal(out["what"], case["what"]) and not np.array_equal(out["where"], case["where"])
    out = refine.reference_step(**{**case, "lr_where": 0.0, "guard_eps": 10.0})     # not even the guard rule touches it
    assert np.array_equal(out["where"], case["where"]) and not np.array_equal(out["what"], case["what"])


def test_guard_rule_on_the_scale_components():
    case = _random_case(5, n=(3, 3, 3, 3))
    case["where"][0, 0] = [0.0, 0.0, -1e-4, 0.0]                   # sx = 0 -> +guard; sy keeps its sign
    case.update(dwhere=np.zeros_like(case["dwhere"]), m_where=np.zeros_like(case["m_where"]), priors=(0.0, 1.0, 0.0, 1e6, 0.0, 1e6),
                lr_where=1e-12)
    out = refine.reference_step(**{**case, "guard_eps": 0.05})
    assert out["where"][0, 0, 0] == 0.05 and out["where"][0, 0, 2] == -0.05
    assert abs(out["where"][0, 0, 1]) < 0.05 and abs(out["where"][0, 0, 3]) < 0.05      # the shifts are not guarded
    big = np.abs(case["where"][..., 0::2]) >= 0.06
    assert np.allclose(out["where"][..., 0::2][big], case["where"][..., 0::2][big], atol=1e-9)
    off = refine.reference_step(**{**case, "guard_eps": 0.0})
    assert abs(off["where"][0, 0, 0]) < 1e-9


# ---- 3. the header and the library ------------------------------------------------------------------------------------------------
def test_prototype_is_in_the_header_on_the_engine_side():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"AIR_ENGINE_API\s+int\s+air_refine_step\s*\(([^;]*)\);", src, flags=re.S)
    assert m, "air_refine_step is not declared AIR_ENGINE_API in include/air_hip.h"
    args = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    from attend_infer_repeat_amd import _lib
    assert len(args) == len(_lib.SIGNATURES["air_refine_step"][1]) == 40
    assert args[0] == "float *what" and args[-1] == "void *stream" and "double *best_J" in args and "int do_update" in args
    assert "refine_kernels.hip" in __import__("attend_infer_repeat_amd.build", fromlist=["SOURCES"]).SOURCES


def test_library_built_here_exports_the_entry_and_checks_its_arguments():
    from attend_infer_repeat_amd import _lib, build
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    assert re.search(r"\bT air_refine_step\b", out)
    lib = _lib.load()
    assert lib.air_abi_version() == 10 and lib.air_engine_abi_version() == 5
    null = [None] * 5 + [1] + [None] * 3 + [0.0, 1.0, 0.0, 1.0, 0.0, 1.0] + [None] * 4 + [1e-2, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.001, 0.0] \
        + [0, 1, 3, 4, 5, 6] + [None] * 6 + [None]
    assert lib.air_refine_step(*null) == -1                        # AIR_E_NULL before any launch (safe without a GPU)
