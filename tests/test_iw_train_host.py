"""Host-only checks of training on the K-particle importance-weighted bound (attend_infer_repeat_amd/iw_train.py): the estimator
is the right one (exact enumeration on a one-latent toy), the float64 restatement of air_iw_vimco, the float32 restatement of
air_iw_logweight_bwd against the closed-form derivative and a finite difference, the refusals, the argument checks of the two
C-ABI entries (they return AIR_E_* before any launch) and the training script's argument errors."""
import ctypes
import itertools
import re
import os

import numpy as np
import pytest

from attend_infer_repeat_amd import iw_train as IT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the estimator -------------------------------------------------------------------------------------------------------------------
# One Bernoulli latent, q(z = 1) = sigmoid(theta), p(x, z) fixed and positive: w(z) = p(x, z) / q(z), so grad log w = -grad log q.
P_JOINT = (0.7, 0.05)              # p(x, z = 0), p(x, z = 1)
THETA = 0.4


def _toy_expected_bound(theta, K):
    """E_q[log (1/K) sum_k w(z_k)] as an exact finite sum; works for a complex theta (complex-step derivative)"""
    s = 1.0 / (1.0 + np.exp(-theta))
    q = (1.0 - s, s)
    total = 0.0
    for zs in itertools.product((0, 1), repeat=K):
        prob = np.prod([q[z] for z in zs])
        total = total + prob * np.log(sum(P_JOINT[z] / q[z] for z in zs) / K)
    return total


def _toy_expected_estimator(theta, K, sign_signal=1.0, sign_weight=1.0):
    """E_q[ sum_k signal_k dlog q(z_k) + sum_k wnorm_k dlog w(z_k) ] with reference_vimco's coefficients, every K-tuple enumerated"""
    s = 1.0 / (1.0 + np.exp(-theta))
    q = (1.0 - s, s)
    dlogq = (-s, 1.0 - s)                                          # d/dtheta log q(z)
    tuples = list(itertools.product((0, 1), repeat=K))
    logw = np.array([[np.log(P_JOINT[z]) - np.log(q[z]) for z in zs] for zs in tuples])
    out = IT.reference_vimco(logw.reshape(-1), K)
    signal, wnorm = out["signal"].reshape(-1, K), out["wnorm"].reshape(-1, K)
    assert not out["degenerate"].any()
    total = 0.0
    for i, zs in enumerate(tuples):
        prob = np.prod([q[z] for z in zs])
        g = sum(sign_signal * signal[i, k] * dlogq[z] + sign_weight * wnorm[i, k] * (-dlogq[z]) for k, z in enumerate(zs))
        total += prob * g
    return total


@pytest.mark.parametrize("K", [2, 3])
def test_vimco_estimator_is_unbiased_for_the_gradient_of_the_bound(K):
    # d/dtheta E[L_K] analytically: the sum is a smooth function of theta, differentiated by the complex step (exact to rounding) ...
    h = 1e-30
    exact = np.imag(_toy_expected_bound(THETA + 1j * h, K)) / h
    # ... and once more by the product rule on the finite sum, L_K itself as the coefficient of dlog q (no control variate)
    s = 1.0 / (1.0 + np.exp(-THETA))
    q, dlogq = (1.0 - s, s), (-s, 1.0 - s)
    rule = 0.0
    for zs in itertools.product((0, 1), repeat=K):
        w = np.array([P_JOINT[z] / q[z] for z in zs])
        rule += np.prod([q[z] for z in zs]) * (np.log(w.mean()) * sum(dlogq[z] for z in zs) + sum(w[k] / w.sum() * -dlogq[z] for k, z in enumerate(zs)))
    assert abs(rule - exact) <= 1e-12 * abs(exact)
    got = _toy_expected_estimator(THETA, K)
    print("K = %d: d E[L_K] / d theta = %.15e, estimator's expectation %.15e" % (K, exact, got))
    assert abs(exact) > 1e-3
    assert abs(got - exact) <= 1e-12 * abs(exact)
    # a sign flip planted on either term breaks it: the signs and the leave-one-out term are pinned
    for flip in (dict(sign_signal=-1.0), dict(sign_weight=-1.0)):
        assert abs(_toy_expected_estimator(THETA, K, **flip) - exact) > 1e-3 * abs(exact), flip


# ---- reference_vimco -------------------------------------------------------------------------------------------------------------------
EPS40 = 2.0 ** -40


def test_reference_vimco_properties():
    rng = np.random.default_rng(0)
    for K in (2, 3, 5, 64, 130):
        lw = rng.uniform(-730.0, -670.0, (4, K))
        out = IT.reference_vimco(lw.reshape(-1), K)
        assert not out["degenerate"].any()
        assert np.abs(out["wnorm"].reshape(4, K).sum(1) - 1.0).max() <= 1e-14
        assert (out["ess"] >= 1.0 - 1e-12).all() and (out["ess"] <= K + 1e-9).all()
        from_scipy = np.logaddexp.reduce(lw, 1) - np.log(K)
        assert np.abs(out["bound"] - from_scipy).max() <= 1e-12 * 730
        # the leave-one-out bound restated particle by particle
        for b in range(4):
            for k in range(K):
                rest = np.delete(lw[b], k)
                loo = np.logaddexp(np.logaddexp.reduce(rest), rest.mean()) - np.log(K)
                assert abs(out["signal"][b * K + k] - (out["bound"][b] - loo)) <= 1e-10
        # a constant added to every log-weight shifts the bound and leaves the coefficients
        moved = IT.reference_vimco((lw + 123.5).reshape(-1), K)
        assert np.abs(moved["bound"] - out["bound"] - 123.5).max() <= EPS40 * 730
        assert np.abs(moved["wnorm"] - out["wnorm"]).max() <= EPS40 and np.abs(moved["signal"] - out["signal"]).max() <= EPS40
    # equal weights: no particle is better than the others' geometric mean
    out = IT.reference_vimco(np.full(3 * 7, -37.25), 7)
    assert np.abs(out["signal"]).max() <= EPS40 and np.abs(out["wnorm"] - 1.0 / 7).max() <= 1e-15
    assert np.abs(out["bound"] + 37.25).max() <= 1e-12 and np.abs(out["ess"] - 7).max() <= 1e-12


def test_reference_vimco_single_minus_inf_and_degenerate_images():
    K = 4
    lw = np.array([[-3.0, -np.inf, -2.0, -4.0],                   # a single -inf: a weight of exactly 0, not degenerate
                   [-1.0, -2.0, np.nan, -3.0],                    # NaN
                   [-1.0, np.inf, -2.0, -3.0],                    # +inf
                   [-np.inf] * 4,                                 # all -inf
                   [-5.0, -6.0, -7.0, -8.0]])                     # a neighbour
    out = IT.reference_vimco(lw.reshape(-1), K)
    assert out["degenerate"].tolist() == [0, 1, 1, 1, 0]
    wn, sg = out["wnorm"].reshape(-1, K), out["signal"].reshape(-1, K)
    for b in (1, 2, 3):
        assert out["bound"][b] == 0.0 and out["ess"][b] == 0.0
        assert not wn[b].any() and not sg[b].any()                # exact zeros
    finite = np.array([-3.0, -2.0, -4.0])
    assert wn[0, 1] == 0.0 and abs(wn[0].sum() - 1.0) <= 1e-15
    assert abs(out["bound"][0] - (np.logaddexp.reduce(finite) - np.log(K))) <= 1e-14
    # particles next to the -inf one: the geometric mean of the others is 0; the -inf one itself is replaced by the others' mean
    assert abs(sg[0, 0] - (out["bound"][0] - (np.logaddexp.reduce(finite[1:]) - np.log(K)))) <= 1e-14
    assert abs(sg[0, 1] - (out["bound"][0] - (np.logaddexp(np.logaddexp.reduce(finite), finite.mean()) - np.log(K)))) <= 1e-14
    assert np.isfinite(sg[0]).all() and np.isfinite(sg[4]).all()
    alone = IT.reference_vimco(lw[4], K)
    for k in ("bound", "ess"):
        assert out[k][4] == alone[k][0]
    assert np.array_equal(wn[4], alone["wnorm"]) and np.array_equal(sg[4], alone["signal"])
    with pytest.raises(ValueError):
        IT.reference_vimco(np.zeros(3), 1)


# ---- reference_logweight_grad --------------------------------------------------------------------------------------------------------
PRIORS = {"fixed": (0.1, 1.3, 0.2, 0.9, -0.15, 1.1), "centred": (0.1, 1.3, 0.2, 0.9, float("nan"), 1.1)}
NAMES = ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale")


def logweight_inputs(T, R, A, seed, counts=None):
    """float32 inputs of the two row entries; counts[r] = n of row r (default: 0, 1, ..., T repeating)"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    a = dict(what=f(T, R, A), what_loc=f(T, R, A), what_scale=(0.3 + 1.7 * rng.random((T, R, A))).astype(np.float32),
             where=f(T, R, 4), where_loc=f(T, R, 4), where_scale=(0.3 + 1.7 * rng.random((T, R, 4))).astype(np.float32),
             g=f(R), rec=(50 + 10 * rng.random(R)).astype(np.float32), logp=(-rng.random(R)).astype(np.float32))
    n = np.arange(R) % (T + 1) if counts is None else np.asarray(counts)
    a["presence"] = (np.arange(T)[:, None] < n[None, :]).astype(np.float32)
    a["n"] = n
    return a


@pytest.mark.parametrize("form", list(PRIORS))
def test_logweight_grad_f32_restatement_against_the_analytic_derivative(form):
    T, R, A = 3, 9, 6
    a = logweight_inputs(T, R, A, seed=3)
    assert set(a["n"].tolist()) == {0, 1, 2, T}
    args = [a[k] for k in NAMES] + [a["presence"], a["g"], PRIORS[form]]
    got = IT.reference_logweight_grad(*args)
    ref = IT.analytic_logweight_grad(*args)
    assert all(g.dtype == np.float32 for g in got)
    for name, g, r in zip(NAMES + ("rec", "logp"), got, ref):
        err = np.abs(g.astype(np.float64) - r).max() / np.abs(r).max()
        print("%s (%s): worst / max = %.3e" % (name, form, err))
        assert err <= 2.0 ** -20, (name, err)
    for g in got[:6]:                                               # rows of steps t >= n are exact zeros
        dead = a["presence"] < 0.5
        assert not g[dead].any() and g[~dead].all()
    assert np.array_equal(got[6], -a["g"]) and np.array_equal(got[7], -a["g"])
    if form == "centred":                                           # the prior term moves with where_loc: d where_loc = -d where there
        assert np.array_equal(got[4][..., 1::2], -got[3][..., 1::2])
        assert not np.array_equal(got[4][..., 0::2], -got[3][..., 0::2])


@pytest.mark.parametrize("form", list(PRIORS))
def test_logweight_grad_against_a_central_difference_of_the_forward(form):
    T, R, A = 3, 8, 5
    a = logweight_inputs(T, R, A, seed=4)
    pr = PRIORS[form]
    table = np.array([0.4, 0.3, 0.2, 0.1])
    x = {k: a[k].astype(np.float64) for k in NAMES}
    rng = np.random.default_rng(5)
    d = {k: rng.standard_normal(x[k].shape) for k in NAMES}
    fwd = lambda h: IT.reference_logweight(*[x[k] + h * d[k] for k in NAMES], a["presence"], a["rec"], a["logp"], table, pr)
    h = 1e-5
    numeric = (fwd(h) - fwd(-h)) / (2 * h)
    grads = IT.analytic_logweight_grad(*[x[k] for k in NAMES], a["presence"], np.ones(R), pr)
    analytic = sum((g * d[k]).reshape(T, R, -1).sum((0, 2)) for k, g in zip(NAMES, grads))
    assert np.abs(analytic).max() > 1.0 and (analytic[a["n"] == 0] == 0).all()
    err = np.abs(numeric - analytic).max() / np.abs(analytic).max()
    print("central difference (%s): worst / max = %.3e" % (form, err))
    assert err <= 1e-6
    # the forward itself: the constant terms are where they belong
    base = fwd(0.0)
    assert np.allclose(base[a["n"] == 0], (-a["rec"].astype(np.float64) + np.log(table[0]) - a["logp"])[a["n"] == 0], rtol=0, atol=1e-12)


def test_zero_scale_stays_in_its_row():
    a = logweight_inputs(3, 5, 6, seed=6, counts=[3, 3, 3, 3, 3])
    args = lambda: [a[k] for k in NAMES] + [a["presence"], a["g"], PRIORS["fixed"]]
    clean = IT.reference_logweight_grad(*args())
    a["what_scale"][1, 2, 3] = 0.0
    hit = IT.reference_logweight_grad(*args())
    assert not np.isfinite(hit[2][1, 2, 3])
    for c, h in zip(clean, hit):
        same = np.ones(c.shape, bool)
        if c.ndim == 3 and c.shape[-1] == 6:
            same[1, 2, 3] = False
        assert np.array_equal(c[same], h[same])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_check_iw_samples():
    assert IT.check_iw_samples(None) is None
    assert IT.check_iw_samples(2) == 2 and IT.check_iw_samples(np.int64(64)) == 64
    with pytest.raises(ValueError, match="default objective"):
        IT.check_iw_samples(1)
    for bad in (0, -4, 2.0, "5", True):
        with pytest.raises(ValueError, match="iw_samples"):
            IT.check_iw_samples(bad)


def test_train_arguments_are_refused_with_a_message():
    P = dict(loc=0.0, scale=1.0)
    ok = dict(decay_rate=None, use_prior=True, discrete_steps=True, what_prior=P, where_scale_prior=P, where_shift_prior=P,
              num_steps_prior=dict(init=0.5))
    assert IT.check_train_arguments(None, **dict(ok, decay_rate=0.9, use_prior=False)) is None      # off: nothing is looked at
    assert IT.check_train_arguments(4, **ok) == 4
    assert IT.check_train_arguments(4, **dict(ok, where_shift_prior=dict(scale=1.0))) == 4           # centred on where_loc: a density
    for change, word in ((dict(decay_rate=0.9), "decay_rate"), (dict(use_prior=False), "use_prior"),
                         (dict(num_steps_prior=None), "num_steps_prior"), (dict(discrete_steps=False), "discrete_steps"),
                         (dict(what_prior=None), "what_prior"), (dict(where_scale_prior=None), "where_scale_prior"),
                         (dict(where_shift_prior=None), "where_shift_prior")):
        with pytest.raises(ValueError, match=word):
            IT.check_train_arguments(4, **dict(ok, **change))
    with pytest.raises(ValueError, match="default objective"):
        IT.check_train_arguments(1, **ok)
    assert IT.priors6(P, dict(loc=0.5, scale=2.0), dict(loc=-1.0, scale=3.0)) == (0.0, 1.0, 0.5, 2.0, -1.0, 3.0)
    assert np.isnan(IT.priors6(P, P, dict(scale=3.0))[4])


def test_training_script_argument_errors(capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    for argv, word in ((["--iw-train", "1"], "default objective"), (["--iw-train", "0"], "iw_samples"),
                       (["--iw-train", "5", "--decay-rate", "0.9"], "--decay-rate"),
                       (["--iw-train", "5", "--iw-particles", "4"], "--iw-particles"),
                       (["--iw-train", "5", "--device-feeder"], "--device-feeder")):
        with pytest.raises(SystemExit):
            multi_mnist.main(argv)
        assert word in capsys.readouterr().err, argv


# ---- the two entries -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


def test_new_entries_are_engine_api_and_the_abi_versions_stay():
    from attend_infer_repeat_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "air_hip.h")).read(), flags=re.S)
    for name, n_args in (("air_iw_logweight_bwd", 27), ("air_iw_vimco", 9)):
        m = re.search(r"AIR_ENGINE_API\s+int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5
    assert re.search(r"#define\s+AIR_ABI_VERSION\s+10\b", src) and re.search(r"#define\s+AIR_ENGINE_ABI_VERSION\s+5\b", src)


def test_new_entries_report_argument_errors(lib):
    f = (ctypes.c_float * 256)()
    i = (ctypes.c_int * 16)()
    F, I = ctypes.cast(f, ctypes.c_void_p), ctypes.cast(i, ctypes.c_void_p)
    pri = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    ins = ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale", "presence", "g")
    outs = ("d_what", "d_what_loc", "d_what_scale", "d_where", "d_where_loc", "d_where_scale", "d_rec", "d_logp")

    def bwd(T=3, R=8, K=4, A=2, **null):
        a = {k: (None if k in null else F) for k in ins + outs}
        return lib.air_iw_logweight_bwd(*[a[k] for k in ins], T, R, K, A, *pri, *[a[k] for k in outs], None)

    def vimco(R=8, K=4, **null):
        a = {k: (None if k in null else F) for k in ("logw", "bound", "wnorm", "signal", "ess")}
        return lib.air_iw_vimco(a["logw"], R, K, a["bound"], a["wnorm"], a["signal"], a["ess"], None if "degenerate" in null else I, None)

    E_NULL, E_SHAPE = -1, -2
    for name in ins + outs:
        assert bwd(**{name: True}) == E_NULL, name
    for name in ("logw", "bound", "wnorm", "signal", "ess", "degenerate"):
        assert vimco(**{name: True}) == E_NULL, name
    assert bwd(K=0) == E_SHAPE and bwd(T=0) == E_SHAPE and bwd(T=33) == E_SHAPE and bwd(R=0) == E_SHAPE and bwd(R=9) == E_SHAPE
    assert bwd(A=0) == E_SHAPE
    assert vimco(K=1) == E_SHAPE and vimco(K=0) == E_SHAPE and vimco(R=0) == E_SHAPE and vimco(R=9) == E_SHAPE
