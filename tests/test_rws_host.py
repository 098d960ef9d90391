"""Host-only checks of training the inference network by reweighted wake-sleep (attend_infer_repeat_amd/iw_train.py,
iw_objective="rws"): the wake-phase update is the right one (exact enumeration on a three-valued toy), the float32 restatement of
air_iw_logposterior_bwd against the closed-form derivative and a finite difference, the refusals, the argument checks of the new
C-ABI entry (it returns AIR_E_* before any launch) and the training script's argument errors."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from attend_infer_repeat_amd import iw_train as IT
from test_iw_train_host import NAMES, logweight_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the estimator -------------------------------------------------------------------------------------------------------------------
# One latent with three values, q = softmax(phi), p(x, z) = exp(theta_z); every K-tuple enumerated, the coefficients reference_rws's.
def _softmax(v):
    e = np.exp(v - v.max())
    return e / e.sum()


def _toy_draws():
    rng = np.random.default_rng(0)
    return [(rng.standard_normal(3), rng.standard_normal(3)) for _ in range(3)]            # (phi, theta), three draws


def _tuples(K):
    return np.array(list(itertools.product(range(3), repeat=K)))                            # [3^K, K]


def _expected_bound(phi, theta, K):
    """E_q[log (1/K) sum_k w(z_k)] as an exact finite sum"""
    q = _softmax(phi)
    zs = _tuples(K)
    w = np.exp(theta)[zs] / q[zs]
    return float((q[zs].prod(1) * np.log(w.mean(1))).sum())


def _expected_wake(phi, theta, K):
    """E_q[sum_k wnorm_k grad_theta log p(x, z_k)] and E_q[sum_k wnorm_k grad_phi log q(z_k)], wnorm from reference_rws"""
    q = _softmax(phi)
    zs = _tuples(K)
    logw = theta[zs] - np.log(q[zs])
    if K == 1:
        wnorm = np.ones((len(zs), 1))                             # a single particle carries all the weight
    else:
        out = IT.reference_rws(logw.reshape(-1), K)
        assert not out["degenerate"].any() and set(out) == {"bound", "wnorm", "ess", "degenerate"}
        wnorm = out["wnorm"].reshape(-1, K)
    prob = q[zs].prod(1)
    onehot = np.eye(3)[zs]                                        # [3^K, K, 3]: grad_theta log p(x, z) = e_z
    g_theta = (prob[:, None] * (wnorm[..., None] * onehot).sum(1)).sum(0)
    g_phi = (prob[:, None] * (wnorm[..., None] * (onehot - q)).sum(1)).sum(0)               # grad_phi log q(z) = e_z - q
    return g_theta, g_phi


@pytest.mark.parametrize("draw", range(3))
def test_wake_theta_update_is_the_gradient_of_the_expected_bound(draw):
    phi, theta = _toy_draws()[draw]
    h = 1e-6
    for K in range(1, 7):
        got = _expected_wake(phi, theta, K)[0]
        numeric = np.array([(_expected_bound(phi, theta + h * e, K) - _expected_bound(phi, theta - h * e, K)) / (2 * h) for e in np.eye(3)])
        err = np.abs(got - numeric).max()
        print("draw %d K = %d: wake-theta against the central difference: %.3e" % (draw, K, err))
        assert err <= 1e-7, (draw, K, err)


@pytest.mark.parametrize("draw", range(3))
def test_wake_phi_update_vanishes_at_the_posterior_and_nears_it_with_K(draw):
    phi, theta = _toy_draws()[draw]
    post = _softmax(theta)                                        # p(z | x)
    for K in (2, 3):                                              # q = p(. | x): every weight equal, nothing to learn
        g = _expected_wake(theta.copy(), theta, K)[1]
        print("draw %d K = %d: wake-phi at q = p(z | x): %.3e" % (draw, K, np.abs(g).max()))
        assert np.abs(g).max() <= 1e-12
    target = post - _softmax(phi)                                 # sum_z p(z | x) grad log q(z)
    dist = [np.abs(_expected_wake(phi, theta, K)[1] - target).max() for K in range(1, 7)]
    print("draw %d: distance of the wake-phi update from p(. | x) - q, K = 1..6: %s" % (draw, ["%.4f" % d for d in dist]))
    assert all(b < a for a, b in zip(dist, dist[1:])), dist


def test_reference_rws_is_reference_vimco_without_the_signal():
    rng = np.random.default_rng(1)
    lw = rng.uniform(-730.0, -670.0, 5 * 4)
    lw[4] = np.nan
    a, b = IT.reference_rws(lw, 4), IT.reference_vimco(lw, 4)
    assert sorted(a) == ["bound", "degenerate", "ess", "wnorm"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["degenerate"].tolist() == [0, 1, 0, 0, 0] and not a["wnorm"].reshape(5, 4)[1].any()


# ---- reference_logposterior_grad -----------------------------------------------------------------------------------------------------
OUT_NAMES = NAMES + ("logp",)


def _inputs(seed, counts=None):
    T, R, A = 3, 6, 5
    a = logweight_inputs(T, R, A, seed=seed, counts=counts)
    assert counts is not None or set(a["n"].tolist()) == {0, 1, 2, 3}
    return T, R, A, a


def test_logposterior_grad_f32_restatement_against_the_analytic_derivative():
    T, R, A, a = _inputs(3)
    args = [a[k] for k in NAMES] + [a["presence"], a["g"]]
    got = IT.reference_logposterior_grad(*args)
    ref = IT.analytic_logposterior_grad(*args)
    assert len(got) == len(ref) == 7 and all(g.dtype == np.float32 for g in got)
    for name, g, r in zip(OUT_NAMES, got, ref):
        err = np.abs(g.astype(np.float64) - r).max() / np.abs(r).max()
        print("%s: worst / max = %.3e" % (name, err))
        assert err <= 2.0 ** -20, (name, err)                      # the bar of the log-weight pair (test_iw_train_host.py)
    dead = a["presence"] < 0.5
    for g in got[:6]:                                               # rows of steps t >= n are exact zeros
        assert not g[dead].any() and g[~dead].all()
    assert np.array_equal(got[6], a["g"])
    assert np.array_equal(got[0], -got[1]) and np.array_equal(got[3], -got[4])       # d x = -d loc, bit for bit


def test_logposterior_grad_against_a_central_difference_of_the_forward():
    T, R, A, a = _inputs(4)
    x = {k: a[k].astype(np.float64) for k in NAMES}
    rng = np.random.default_rng(5)
    d = {k: rng.standard_normal(x[k].shape) for k in NAMES}
    fwd = lambda h: IT.reference_logposterior(*[x[k] + h * d[k] for k in NAMES], a["presence"], a["logp"])
    h = 1e-5
    numeric = (fwd(h) - fwd(-h)) / (2 * h)
    grads = IT.analytic_logposterior_grad(*[x[k] for k in NAMES], a["presence"], np.ones(R))
    analytic = sum((g * d[k]).reshape(T, R, -1).sum((0, 2)) for k, g in zip(NAMES, grads))
    assert np.abs(analytic).max() > 1.0 and (analytic[a["n"] == 0] == 0).all()
    err = np.abs(numeric - analytic).max() / np.abs(analytic).max()
    print("central difference: worst / max = %.3e" % err)
    assert err <= 1e-6
    # the forward itself: logp where nothing is present, and every term with its -1/2 log 2 pi
    base = fwd(0.0)
    assert np.allclose(base[a["n"] == 0], a["logp"].astype(np.float64)[a["n"] == 0], rtol=0, atol=1e-12)
    r = int(np.flatnonzero(a["n"] == 2)[0])
    N = lambda v, l, s: -0.5 * ((v - l) / s) ** 2 - np.log(s) - 0.5 * np.log(2 * np.pi)
    by_hand = a["logp"][r] + sum(N(x["what"][t, r], x["what_loc"][t, r], x["what_scale"][t, r]).sum()
                                 + N(x["where"][t, r], x["where_loc"][t, r], x["where_scale"][t, r]).sum() for t in range(2))
    assert abs(base[r] - by_hand) <= 1e-12 * abs(by_hand)
    # d logp = g
    assert np.array_equal(IT.analytic_logposterior_grad(*[x[k] for k in NAMES], a["presence"], a["g"])[6], a["g"].astype(np.float64))


def test_zero_scale_stays_in_its_row():
    T, R, A, a = _inputs(6, counts=[3] * 6)
    args = lambda: [a[k] for k in NAMES] + [a["presence"], a["g"]]
    clean = IT.reference_logposterior_grad(*args())
    a["what_scale"][1, 2, 3] = 0.0
    a["where_scale"][2, 4, 1] = 0.0
    hit = IT.reference_logposterior_grad(*args())
    assert not np.isfinite(hit[2][1, 2, 3]) and not np.isfinite(hit[5][2, 4, 1])
    for c, h in zip(clean, hit):
        same = np.ones(c.shape, bool)
        if c.ndim == 3 and c.shape[-1] == A:
            same[1, 2, 3] = False
        elif c.ndim == 3:
            same[2, 4, 1] = False
        assert np.array_equal(c[same], h[same])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_iw_objective_is_checked_with_a_message():
    P = dict(loc=0.0, scale=1.0)
    ok = dict(decay_rate=None, use_prior=True, discrete_steps=True, what_prior=P, where_scale_prior=P, where_shift_prior=P,
              num_steps_prior=dict(init=0.5))
    # None / "vimco": what the call returned before
    assert IT.check_train_arguments(None, **dict(ok, decay_rate=0.9, use_prior=False)) is None
    assert IT.check_train_arguments(None, iw_objective=None, **ok) is None
    for obj in (None, "vimco"):
        assert IT.check_train_arguments(4, iw_objective=obj, **ok) == 4
        assert IT.check_train_arguments(4, iw_objective=obj, use_reinforce=False, **ok) == 4
        with pytest.raises(ValueError, match="decay_rate"):
            IT.check_train_arguments(4, iw_objective=obj, **dict(ok, decay_rate=0.9))
    assert IT.check_train_arguments(2, iw_objective="rws", **ok) == 2
    assert IT.check_iw_objective(None, None) is None and IT.check_iw_objective(None, 4) == "vimco"
    assert IT.check_iw_objective("vimco", 4) == "vimco" and IT.check_iw_objective("rws", 2) == "rws"
    # "rws" needs iw_samples >= 2 ...
    with pytest.raises(ValueError, match="iw_samples >= 2"):
        IT.check_train_arguments(1, iw_objective="rws", **ok)
    for obj in ("rws", "vimco"):                                    # ... and an objective without iw_samples is refused
        with pytest.raises(ValueError, match="needs iw_samples"):
            IT.check_train_arguments(None, iw_objective=obj, **ok)
    with pytest.raises(ValueError, match="use_reinforce=False"):
        IT.check_train_arguments(4, iw_objective="rws", use_reinforce=False, **ok)
    for bad in ("RWS", "iwae", 1, True):
        with pytest.raises(ValueError, match="iw_objective must be"):
            IT.check_train_arguments(4, iw_objective=bad, **ok)
    with pytest.raises(ValueError, match="use_prior"):              # the other refusals hold under "rws" too
        IT.check_train_arguments(4, iw_objective="rws", **dict(ok, use_prior=False))


def test_training_script_argument_errors(capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    for argv, word in ((["--iw-objective", "rws"], "--iw-train"), (["--iw-objective", "vimco"], "--iw-train"),
                       (["--iw-train", "2", "--iw-objective", "iwae"], "invalid choice"),
                       (["--iw-train", "1", "--iw-objective", "rws"], "default objective"),
                       (["--iw-train", "5", "--iw-objective", "rws", "--decay-rate", "0.9"], "--decay-rate")):
        with pytest.raises(SystemExit):
            multi_mnist.main(argv)
        assert word in capsys.readouterr().err, argv


# ---- the entry ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import _lib, build
    build.build()
    return _lib.load()


def test_new_entry_is_engine_api_and_the_abi_versions_stay():
    from attend_infer_repeat_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "air_hip.h")).read(), flags=re.S)
    m = re.search(r"AIR_ENGINE_API\s+int\s+air_iw_logposterior_bwd\s*\(([^;]*)\);", src, flags=re.S)
    assert m
    assert len(m.group(1).split(",")) == 20 == len(_lib.SIGNATURES["air_iw_logposterior_bwd"][1])
    assert _lib.SIGNATURES["air_iw_logposterior_bwd"][0] is ctypes.c_int
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5
    assert re.search(r"#define\s+AIR_ABI_VERSION\s+10\b", src) and re.search(r"#define\s+AIR_ENGINE_ABI_VERSION\s+5\b", src)


def test_new_entry_reports_argument_errors(lib):
    f = (ctypes.c_float * 256)()
    base = ctypes.addressof(f)
    base += (-base) % 16                                            # a 16-byte aligned start inside the block
    F, OFF4 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    ins = ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale", "presence", "g")
    outs = ("d_what", "d_what_loc", "d_what_scale", "d_where", "d_where_loc", "d_where_scale", "d_logp")

    def bwd(T=3, R=8, K=4, A=2, **ptr):
        a = {k: ptr.get(k, F) for k in ins + outs}
        return lib.air_iw_logposterior_bwd(*[a[k] for k in ins], T, R, K, A, *[a[k] for k in outs], None)

    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    for name in ins + outs:
        if name in ("d_what", "d_where"):                           # optional: a NULL is not a NULL error
            continue
        assert bwd(**{name: None}) == E_NULL, name
    assert bwd(K=0) == E_SHAPE and bwd(T=0) == E_SHAPE and bwd(T=33) == E_SHAPE and bwd(R=0) == E_SHAPE and bwd(R=9) == E_SHAPE
    assert bwd(A=0) == E_SHAPE
    assert bwd(T=33, d_what=None, d_where=None) == E_SHAPE          # the optional outputs left out: the checks behind them still run
    for name in ("where", "where_loc", "where_scale", "d_where", "d_where_loc", "d_where_scale"):
        assert bwd(**{name: OFF4}) == E_ALIGN, name
    assert bwd(where=OFF4, d_what=None, d_where=None) == E_ALIGN
