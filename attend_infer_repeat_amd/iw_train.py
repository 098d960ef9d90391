"""Training on the K-particle importance-weighted bound (IWAE weights for the continuous latents, VIMCO's leave-one-out signal for
the discrete count): the host side.  Pure numpy, importable and callable without a GPU.

    L_K(x) = log (1/K) sum_k w_k,   w_k = p(x, z_k) / q(z_k | x),   z_k ~ q(. | x)   (rows r = b * K + k, iw_eval.py)

The gradient estimator of -mean_b L_K (Mnih & Rezende 2016, "Variational inference for Monte Carlo objectives"), per image:

    sum_k wnorm_k grad log w_k  +  sum_k signal_k grad log q(n_k | x)
    wnorm_k  = w_k / sum_j w_j
    signal_k = L_K - L_K(-k),   L_K(-k) = log (1/K) (sum_{j != k} w_j + what_k),   log what_k = (1/(K-1)) sum_{j != k} log w_j

wnorm and signal are constants of the backward pass.  grad log w_k goes through the reparameterised what / where samples and the
densities' own parameters (air_iw_logweight_bwd); log q(n_k | x) is F.numsteps' log-probability of the sampled count.

DEGENERATE images: a NaN or +inf log-weight, or all K at -inf.  Their wnorm and signal rows are exact zeros, their bound and ess
are 0 and they take no part in the step (the mean is over the others).  A single -inf among finite log-weights is a weight of
exactly 0 and follows the plain formulas; at K = 2 the surviving particle's signal is then +inf.

This module restates the two device entries (include/air_hip.h: air_iw_vimco, air_iw_logweight_bwd):
  reference_vimco           numpy float64, the leave-one-out sums formed directly (K^2 terms per image);
  reference_logweight_grad  numpy float32 (or any dtype), operation by operation in the kernel's order: the kernel's bits;
  analytic_logweight_grad   the same gradient in float64 from the closed-form derivative of the densities;
  reference_logweight       the forward value in float64 (what a finite difference is taken of).

iw_objective="rws" trains on the same particles by the wake-phase update of reweighted wake-sleep instead (Bornschein & Bengio 2015;
Le et al. 2019): sum_k wnorm_k grad log q(z_k | x) for the inference network and sum_k wnorm_k grad log p(x, z_k) for the decoder,
z_k fixed values, wnorm_k constants, no signal term.  reference_rws, reference_logposterior_grad, analytic_logposterior_grad and
reference_logposterior restate its entry (air_iw_logposterior_bwd) the same way.
"""
import numpy as np

IW_SAMPLES_ONE = ("iw_samples=1 is the single-sample bound: use the default objective (iw_samples=None: ELBO with the NVIL "
                  "baseline) for it; the importance-weighted objective needs iw_samples >= 2")
NO_DECAY_RATE = ("iw_samples: decay_rate normalises the NVIL importance weight, which the importance-weighted objective does not "
                 "have (its learning signal is VIMCO's leave-one-out difference); leave decay_rate at None")
NEEDS_PRIOR = ("iw_samples: use_prior=False removes the generative density the importance weight is a ratio of; the importance-"
               "weighted objective needs use_prior=True")
NEEDS_STEPS_PRIOR = "iw_samples: num_steps_prior is needed (log pi(n) is a term of the importance weight)"
IW_OBJECTIVES = ("vimco", "rws")
OBJECTIVE_NEEDS_SAMPLES = ("iw_objective chooses the estimator of the K-particle objective and needs iw_samples >= 2; without iw_samples "
                           "the default objective (ELBO with the NVIL baseline) is trained and iw_objective must stay None")
RWS_NEEDS_LOGQ = ('iw_objective="rws": use_reinforce=False switches off a score-function term, and the wake-phase update has none -- '
                  "log q(n | x) is part of its target log q(z | x); leave use_reinforce at True")


def check_iw_samples(K):
    """None: off (returns None).  An int >= 2: accepted (returns it).  1 and anything else: ValueError."""
    if K is None:
        return None
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)):
        raise ValueError("iw_samples must be None or an integer >= 2, got %r" % (K,))
    if int(K) == 1:
        raise ValueError(IW_SAMPLES_ONE)
    if int(K) < 2:
        raise ValueError("iw_samples must be None or an integer >= 2, got %r" % (K,))
    return int(K)


def check_iw_objective(iw_objective, K, use_reinforce=True):
    """None / "vimco": the VIMCO estimator (returns "vimco", or None when K is None).  "rws": the wake-phase update of reweighted
    wake-sleep; needs K >= 2 and use_reinforce.  An objective without iw_samples, or any other value: ValueError."""
    if iw_objective is not None and iw_objective not in IW_OBJECTIVES:
        raise ValueError("iw_objective must be None, %s, got %r" % (" or ".join(repr(o) for o in IW_OBJECTIVES), iw_objective))
    if K is None:
        if iw_objective is not None:
            raise ValueError(OBJECTIVE_NEEDS_SAMPLES)
        return None
    if iw_objective == "rws" and not use_reinforce:
        raise ValueError(RWS_NEEDS_LOGQ)
    return iw_objective or "vimco"


def check_train_arguments(K, decay_rate, use_prior, discrete_steps, what_prior, where_scale_prior, where_shift_prior, num_steps_prior,
                          iw_objective=None, use_reinforce=True):
    """What train_step(iw_samples=K) refuses, each with a message (ValueError); the prior configuration by iw_eval.check_config's rules.
    Returns K; `iw_objective` (None / "vimco": nothing changes; "rws") is checked by check_iw_objective."""
    K = check_iw_samples(K)
    check_iw_objective(iw_objective, K, use_reinforce)
    if K is None:
        return None
    if decay_rate is not None:
        raise ValueError(NO_DECAY_RATE)
    if not use_prior:
        raise ValueError(NEEDS_PRIOR)
    if num_steps_prior is None:
        raise ValueError(NEEDS_STEPS_PRIOR)
    from types import SimpleNamespace
    from .iw_eval import check_config
    check_config(SimpleNamespace(discrete_steps=bool(discrete_steps), what_prior=what_prior, where_scale_prior=where_scale_prior,
                                 where_shift_prior=where_shift_prior), K)
    return K


def priors6(what_prior, where_scale_prior, where_shift_prior):
    """the six prior scalars of air_iw_logweight from train_step's three prior dicts; a shift prior without `loc` -> NaN (centred on where_loc)"""
    shift_loc = where_shift_prior["loc"] if "loc" in where_shift_prior else float("nan")
    return (float(what_prior["loc"]), float(what_prior["scale"]), float(where_scale_prior["loc"]), float(where_scale_prior["scale"]),
            float(shift_loc), float(where_shift_prior["scale"]))


# ---- air_iw_vimco -------------------------------------------------------------------------------------------------------------------
def reference_vimco(logw, K):
    """logw: R = B * K log-weights (row b * K + k).  Returns float64 bound[B], wnorm[R], signal[R], ess[B] and int degenerate[B]."""
    lw = np.asarray(logw, np.float64).reshape(-1, int(K))
    B, K = lw.shape
    if K < 2:
        raise ValueError("reference_vimco needs K >= 2")
    bound, ess, degen = np.zeros(B), np.zeros(B), np.zeros(B, np.int32)
    wnorm, signal = np.zeros((B, K)), np.zeros((B, K))
    off = ~np.eye(K, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            v = lw[b]
            if np.isnan(v).any() or (v == np.inf).any() or (v == -np.inf).all():
                degen[b] = 1
                continue
            m = v.max()
            e = np.exp(v - m)
            S = e.sum()
            bound[b] = m + np.log(S) - np.log(K)
            ess[b] = S * S / (e * e).sum()
            wnorm[b] = e / S
            loo = np.where(off, e[None, :], 0.0).sum(1)                       # sum_{j != k} e_j, formed directly
            lgeo = np.where(off, v[None, :], 0.0).sum(1) / (K - 1)            # (1/(K-1)) sum_{j != k} lw_j
            signal[b] = np.log(S) - np.log(loo + np.exp(lgeo - m))            # bound - bound without k: m and log K cancel
    return dict(bound=bound, wnorm=wnorm.reshape(-1), signal=signal.reshape(-1), ess=ess, degenerate=degen)


# ---- air_iw_logweight and its backward ------------------------------------------------------------------------------------------------
def leading_ones(presence):
    """n[R]: the number of leading ones of the presence chain [T, R] (or [T, R, 1])"""
    z = np.asarray(presence)
    z = z.reshape(z.shape[0], -1) > 0.5
    return np.cumprod(z, 0).sum(0).astype(np.int64)


def _prior_columns(where_loc, pr, dtype):
    """p_loc, p_scale [T, R, 4] of the where components and whether the shift prior is centred on where_loc"""
    centred = pr[4] != pr[4]
    p_loc = np.empty_like(where_loc)
    p_loc[..., 0::2] = dtype(pr[2])
    p_loc[..., 1::2] = where_loc[..., 1::2] if centred else dtype(pr[4])
    p_scale = np.empty_like(where_loc)
    p_scale[..., 0::2] = dtype(pr[3])
    p_scale[..., 1::2] = dtype(pr[5])
    return p_loc, p_scale, centred


def reference_logweight_grad(what, what_loc, what_scale, where, where_loc, where_scale, presence, g, priors, dtype=np.float32):
    """air_iw_logweight_bwd operation by operation in `dtype` (float32: the kernel's bits).  Returns the eight outputs in the entry's
    order: d what, d what_loc, d what_scale [T,R,A], d where, d where_loc, d where_scale [T,R,4], d rec [R], d logp [R]."""
    dt = np.dtype(dtype).type
    c = lambda a: np.ascontiguousarray(np.asarray(a), dtype=dt)
    what, what_loc, what_scale, where, where_loc, where_scale, g = (c(a) for a in (what, what_loc, what_scale, where, where_loc,
                                                                                  where_scale, g))
    T, R = what.shape[:2]
    n = leading_ones(presence)
    live = (np.arange(T)[:, None] < n[None, :])[..., None]                     # [T, R, 1]
    gr = g.reshape(1, R, 1)
    one, zero = dt(1), dt(0)

    def grads(x, loc, scale, p_loc, p_scale, centred_cols):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            zq = (x - loc) / scale
            zp = (x - p_loc) / p_scale
            a = zq / scale
            b = zp / p_scale
            dx = gr * (a - b)
            dloc = gr * (np.where(centred_cols, b, zero) - a)
            dscale = gr * ((one - zq * zq) / scale)
        return tuple(np.where(live, d, zero).astype(dt) for d in (dx, dloc, dscale))

    dwhat = grads(what, what_loc, what_scale, dt(priors[0]), dt(priors[1]), False)
    p_loc, p_scale, centred = _prior_columns(where_loc, priors, dt)
    cols = np.zeros(4, bool)
    cols[1::2] = centred
    dwhere = grads(where, where_loc, where_scale, p_loc, p_scale, cols.reshape(1, 1, 4))
    return dwhat + dwhere + ((-g).astype(dt), (-g).astype(dt))


def analytic_logweight_grad(what, what_loc, what_scale, where, where_loc, where_scale, presence, g, priors):
    """The same eight gradients in float64 from the closed-form derivative of log N(x | p) - log N(x | q):
    d/dx = (x - loc) / scale^2 - (x - p_loc) / p_scale^2;  d/dloc = -(x - loc) / scale^2 (+ (x - p_loc) / p_scale^2 when the prior is
    centred on loc);  d/dscale = 1 / scale - (x - loc)^2 / scale^3."""
    f = lambda a: np.asarray(a, np.float64)
    what, what_loc, what_scale, where, where_loc, where_scale, g = (f(a) for a in (what, what_loc, what_scale, where, where_loc,
                                                                                  where_scale, g))
    T, R = what.shape[:2]
    live = (np.arange(T)[:, None] < leading_ones(presence)[None, :])[..., None]
    gr = g.reshape(1, R, 1)

    def grads(x, loc, scale, p_loc, p_scale, centred_cols):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = (x - loc) / scale ** 2
            p = (x - p_loc) / p_scale ** 2
            out = (gr * (q - p), gr * (np.where(centred_cols, p, 0.0) - q), gr * (1.0 / scale - (x - loc) ** 2 / scale ** 3))
        return tuple(np.where(live, d, 0.0) for d in out)

    dwhat = grads(what, what_loc, what_scale, priors[0], priors[1], False)
    p_loc, p_scale, centred = _prior_columns(where_loc, priors, np.float64)
    cols = np.zeros(4, bool)
    cols[1::2] = centred
    return dwhat + grads(where, where_loc, where_scale, p_loc, p_scale, cols.reshape(1, 1, 4)) + (-g, -g)


def reference_logweight(what, what_loc, what_scale, where, where_loc, where_scale, presence, rec, logp, prior_table, priors,
                        normalize=False):
    """air_iw_logweight's row value in float64: -rec + log pi(n) - logp + sum_{t<n} (sum_a log p/q (what) + sum_j log p/q (where))"""
    f = lambda a: np.asarray(a, np.float64)
    what, what_loc, what_scale, where, where_loc, where_scale = (f(a) for a in (what, what_loc, what_scale, where, where_loc,
                                                                               where_scale))
    T = what.shape[0]
    n = leading_ones(presence)
    live = np.arange(T)[:, None] < n[None, :]

    def ratio(x, loc, scale, p_loc, p_scale):
        zq, zp = (x - loc) / scale, (x - p_loc) / p_scale
        return (0.5 * (zq * zq - zp * zp) + (np.log(scale) - np.log(p_scale))).sum(-1)

    p_loc, p_scale, _ = _prior_columns(where_loc, priors, np.float64)
    s = ratio(what, what_loc, what_scale, priors[0], priors[1]) + ratio(where, where_loc, where_scale, p_loc, p_scale)
    table = f(prior_table)
    if normalize:
        table = table / table.sum()
    return -f(rec) + np.log(table)[n] - f(logp) + np.where(live, s, 0.0).sum(0)


# ---- reweighted wake-sleep: air_iw_logposterior and its backward -----------------------------------------------------------------------
def reference_rws(logw, K):
    """The coefficients of the wake-phase update: reference_vimco's bound[B], wnorm[R], ess[B] and degenerate[B] (wnorm_k multiplies
    grad log q(z_k | x) and grad log p(x, z_k); VIMCO's signal is not used)."""
    out = reference_vimco(logw, K)
    return {k: out[k] for k in ("bound", "wnorm", "ess", "degenerate")}


def reference_logposterior_grad(what, what_loc, what_scale, where, where_loc, where_scale, presence, g, dtype=np.float32):
    """air_iw_logposterior_bwd operation by operation in `dtype` (float32: the kernel's bits).  Returns the seven outputs in the entry's
    order: d what, d what_loc, d what_scale [T,R,A], d where, d where_loc, d where_scale [T,R,4], d logp [R]."""
    dt = np.dtype(dtype).type
    c = lambda a: np.ascontiguousarray(np.asarray(a), dtype=dt)
    what, what_loc, what_scale, where, where_loc, where_scale, g = (c(a) for a in (what, what_loc, what_scale, where, where_loc,
                                                                                  where_scale, g))
    T, R = what.shape[:2]
    live = (np.arange(T)[:, None] < leading_ones(presence)[None, :])[..., None]       # [T, R, 1]
    gr = g.reshape(1, R, 1)
    one, zero = dt(1), dt(0)

    def grads(x, loc, scale):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            zq = (x - loc) / scale
            a = zq / scale
            dloc = gr * a
            dscale = gr * ((zq * zq - one) / scale)
            dx = gr * (zero - a)
        return tuple(np.where(live, d, zero).astype(dt) for d in (dx, dloc, dscale))

    return grads(what, what_loc, what_scale) + grads(where, where_loc, where_scale) + (g.copy(),)


def analytic_logposterior_grad(what, what_loc, what_scale, where, where_loc, where_scale, presence, g):
    """The same seven gradients in float64 from the closed-form derivative of log N(x | loc, scale):
    d/dx = -(x - loc) / scale^2;  d/dloc = (x - loc) / scale^2;  d/dscale = (x - loc)^2 / scale^3 - 1 / scale."""
    f = lambda a: np.asarray(a, np.float64)
    what, what_loc, what_scale, where, where_loc, where_scale, g = (f(a) for a in (what, what_loc, what_scale, where, where_loc,
                                                                                  where_scale, g))
    T, R = what.shape[:2]
    live = (np.arange(T)[:, None] < leading_ones(presence)[None, :])[..., None]
    gr = g.reshape(1, R, 1)

    def grads(x, loc, scale):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = (x - loc) / scale ** 2
            out = (gr * -q, gr * q, gr * ((x - loc) ** 2 / scale ** 3 - 1.0 / scale))
        return tuple(np.where(live, d, 0.0) for d in out)

    return grads(what, what_loc, what_scale) + grads(where, where_loc, where_scale) + (g.copy(),)


def reference_logposterior(what, what_loc, what_scale, where, where_loc, where_scale, presence, logp):
    """air_iw_logposterior's row value in float64: logp + sum_{t<n} (sum_a log N(what) + sum_j log N(where)), every term with its
    -1/2 log 2 pi"""
    f = lambda a: np.asarray(a, np.float64)
    what, what_loc, what_scale, where, where_loc, where_scale = (f(a) for a in (what, what_loc, what_scale, where, where_loc,
                                                                               where_scale))
    T = what.shape[0]
    live = np.arange(T)[:, None] < leading_ones(presence)[None, :]

    def log_normal(x, loc, scale):
        zq = (x - loc) / scale
        return (-0.5 * (zq * zq) - np.log(scale) - 0.5 * np.log(2.0 * np.pi)).sum(-1)

    s = log_normal(what, what_loc, what_scale) + log_normal(where, where_loc, where_scale)
    return f(logp) + np.where(live, s, 0.0).sum(0)
