"""GPU tests of parse refinement (attend_infer_repeat_amd/refine.py, csrc/refine_kernels.hip): air_refine_step alone against
refine.reference_step (numpy float64) on the kernel's own fp32 inputs, then ParseRefiner behind a SceneParser / ParticleParser: its
gradients and its trajectory against float64 autograd through the oracle's decoder, canvas write and reconstruction term, the keep
rule on the device's own numbers, steps = 0 against the bound parser, graph replay against eager, scoring, and the public surface.

Bars.  J is -rec plus a sum of per-sample log densities, the kind of number log w is: test_iw_eval.py's OUT_TOL = 1e-4 (worst element
/ tensor max) and OUT_L2 = 3e-5 (relative L2).  An updated latent or moment is about ten fp32 roundings of numbers no larger than
its own inputs (z, the gradient, the prior location, m, v): 16 ulp of max(|ref|, |those inputs|).  Gradients: test_engine.py's
GRAD_TOL = 3e-4 / GRAD_L2 = 2e-4.  Trajectory: with eps = 1 one Adam step is Lipschitz in the gradient with constant
<= lr, so after `steps` steps the device may be off by about steps * lr * |dg|, |dg| = GRAD_TOL * max|g|; the bar is 4x that.  The
trace is J at those latents: OUT_TOL * max|J| for the evaluation plus (the largest per-image L1 norm of g) * (the latent bar) for the
displacement."""
import dataclasses
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from oracle import air_oracle as O
from test_engine import CONFIGS, GRAD_L2, GRAD_TOL, OUT_L2, OUT_TOL, check_tensor, f64
from test_parse import MASK_THRESHOLD, SENTINEL_F, SENTINEL_I, _mnist_air, _train_state, e2e_case, engine_config, make_parser

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))                               # a launch argument as the kernel receives it (a C float)
ADAM = dict(beta1=F32(0.9), beta2=F32(0.999), eps=F32(1e-8))       # the references get the kernel's own fp32 inputs
MOVING = ("what", "where", "m_what", "v_what", "m_where", "v_where")


def same_bits(a, b):
    """torch.equal that lets NaN equal NaN"""
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0),
                                                                                                  torch.nan_to_num(b, nan=0.0))
    return torch.equal(a, b)


# ---- 1. air_refine_step alone -----------------------------------------------------------------------------------------------------
def step_case(T, B, A, G, seed, n=None, n_bands=3):
    """fp32 inputs of one call as numpy arrays; n[b] = the number of present steps (default: random, 0 and T included when B allows)"""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)
    if n is None:
        n = rng.integers(0, T + 1, B)
        n[0] = T
        if B > 1:
            n[1] = 0
    presence = (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(np.float32)
    return dict(what=r(T, B, A), where=r(T, B, 4), glimpse=r(T, B, G), presence=presence, rec_parts=np.abs(r(n_bands, B)) * 50,
                dwhat=r(T, B, A) * 3, dwhere=r(T, B, 4) * 30, where_loc=r(T, B, 4), m_what=r(T, B, A), v_what=np.abs(r(T, B, A)),
                m_where=r(T, B, 4), v_where=np.abs(r(T, B, 4)))


def run_step(case, priors, lr_what, lr_where, c1, c2, guard_eps, iter, do_update, best=None, trace_rows=None, beta1=0.9, beta2=0.999,
             eps=1e-8, no_trace=False):
    """air_refine_step alone on device copies of `case` (current stream).  Outputs start as sentinel fills unless `best` (device
    tensors of a previous call) is handed in.  Returns (the device tensors after the call: in/out latents, moments, best_*, J_trace,
    the status).  no_trace: J_trace = NULL and where_loc = NULL are handed to the entry (for a given shift loc; the trace buffer stays in the
    result, untouched)"""
    from attend_infer_repeat_amd import hip as Hh
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items()}
    T, B, A = d["what"].shape
    G = d["glimpse"].shape[-1]
    if best is None:
        best = dict(best_J=torch.full((B,), SENTINEL_F, dtype=torch.float64).cuda(),
                    best_iter=torch.full((B,), SENTINEL_I, dtype=torch.int32).cuda(),
                    best_what=torch.full((T, B, A), SENTINEL_F).cuda(), best_where=torch.full((T, B, 4), SENTINEL_F).cuda(),
                    best_glimpse=torch.full((T, B, G), SENTINEL_F).cuda(),
                    J_trace=torch.full((trace_rows or iter + 1, B), SENTINEL_F).cuda())
    d.update(best)
    p = Hh._p
    pl = [float("nan") if v is None else float(v) for v in priors]
    st = Hh.lib().air_refine_step(p(d["what"]), p(d["where"]), p(d["glimpse"]), p(d["presence"]), p(d["rec_parts"]),
                                  d["rec_parts"].shape[0], p(d["dwhat"]), p(d["dwhere"]), None if no_trace else p(d["where_loc"]), *pl, p(d["m_what"]),
                                  p(d["v_what"]), p(d["m_where"]), p(d["v_where"]), lr_what, lr_where, beta1, beta2, eps, c1, c2,
                                  guard_eps, iter, do_update, T, B, A, G, p(d["best_J"]), p(d["best_iter"]), p(d["best_what"]),
                                  p(d["best_where"]), p(d["best_glimpse"]), None if no_trace else p(d["J_trace"]), Hh._stream())
    torch.cuda.synchronize()
    return d, st


def ulp_excess(got, ref, *inputs):
    """max over the elements of |got - ref| / ulp32(max(|ref|, |inputs|)) (0 where both are the same non-finite value)"""
    scale = np.abs(ref)
    for x in inputs:
        scale = np.maximum(scale, np.abs(np.broadcast_to(x, ref.shape).astype(np.float64)))
    ulp = np.spacing(np.maximum(scale, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - ref) / ulp).max()) if ref.size else 0.0


def prior_means(case, priors):
    mu = np.empty_like(case["where"])
    mu[..., 0::2] = priors[2]
    mu[..., 1::2] = case["where_loc"][..., 1::2] if priors[4] is None else priors[4]
    return mu


@pytest.mark.parametrize("shift_loc", [0.25, None])
@pytest.mark.parametrize("A,G", [(50, 400), (7, 9), (12, 16)])      # 8-byte / 4-byte / 16-byte loads of `what`; both copy paths
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [1, 3, 32])
def test_step_matches_reference_step(gpu_device, T, B, A, G, shift_loc):
    """Worst observed on an MI355X over all 36 cases: an updated latent or moment 0.62 ulp off the float64 rule (T3_B1_A12_G16; every
    case between 0.42 and 0.62; bar 16 ulp)."""
    from attend_infer_repeat_amd import refine
    priors = (0.1, 1.5, 1.0, 0.5, shift_loc, 2.0)
    case = step_case(T, B, A, G, seed=100 * T + 10 * B + A)
    it, lr = 2, (F32(1e-2), F32(3e-2))
    c1, c2 = F32(1 - 0.9 ** (it + 1)), F32(1 - 0.999 ** (it + 1))
    # a best-so-far that some images beat and some do not (float64, NaN for one image when B allows)
    ref0 = refine.reference_step(**case, priors=priors, lr_what=lr[0], lr_where=lr[1], **ADAM, c1=c1, c2=c2, guard_eps=0.0, iter=it,
                                 do_update=0, best=None)
    prev_J = ref0["J"] + np.where(np.arange(B) % 2 == 0, -4.0, 4.0)
    if B > 2:
        prev_J[2] = np.nan
    mk = lambda shape, v, dt=torch.float32: torch.full(shape, v, dtype=dt).cuda()
    best = dict(best_J=torch.from_numpy(prev_J).cuda(), best_iter=mk((B,), 1, torch.int32), best_what=mk((T, B, A), 7.0),
                best_where=mk((T, B, 4), 7.0), best_glimpse=mk((T, B, G), 7.0), J_trace=mk((it + 1, B), SENTINEL_F))
    prev = {"J": prev_J, "iter": np.ones(B, np.int64), "what": np.full((T, B, A), 7.0), "where": np.full((T, B, 4), 7.0),
            "glimpse": np.full((T, B, G), 7.0)}
    ref = refine.reference_step(**case, priors=priors, lr_what=lr[0], lr_where=lr[1], **ADAM, c1=c1, c2=c2, guard_eps=0.0, iter=it,
                                do_update=1, best=prev)
    got, st = run_step(case, priors, lr[0], lr[1], c1, c2, 0.0, it, 1, best=best)
    assert st == 0
    name = "T%d_B%d_A%d_G%d_%s" % (T, B, A, G, "given" if shift_loc is not None else "centred")
    J = got["J_trace"][it].cpu()
    check_tensor("refine_step", name, "out", "J", J, torch.from_numpy(ref["J"]), OUT_TOL, OUT_L2)
    assert (got["J_trace"][:it] == SENTINEL_F).all()               # only this iteration's row is written
    # the keep rule on the DEVICE's J (float64 best_J = its own J where taken), then bit copies
    Jd = got["best_J"].cpu().numpy()
    take = got["best_iter"].cpu().numpy() == it
    assert np.abs(ref["J"]).max() * OUT_TOL < 2.0                  # the crafted gap is 4: the J bar settles every image
    assert np.array_equal(take, ref["take"]) and take[0] and (B < 2 or not take[1]) and (B < 3 or take[2])
    assert np.array_equal(got["best_iter"].cpu().numpy(), np.where(take, it, 1))
    assert np.array_equal(Jd[~take], prev_J[~take], equal_nan=True)
    assert np.array_equal(np.float32(Jd[take]), J.numpy()[take])
    for k in ("what", "where", "glimpse"):
        want = np.where(take[None, :, None], case[k], np.float32(7.0))
        assert np.array_equal(got["best_" + k].cpu().numpy(), want), k
    # the update: rows t >= n bit-identical, the others within 16 ulp
    mask = case["presence"] > 0.5
    mu = prior_means(case, priors)
    worst = 0.0
    for k in MOVING:
        g = got[k].cpu().numpy()
        assert np.array_equal(g[~mask], case[k][~mask]), k
        grp = "what" if k.endswith("what") else "where"
        ins = [case[grp], case["d" + grp], case["m_" + grp], case["v_" + grp], priors[0] if grp == "what" else mu]
        worst = max(worst, ulp_excess(g[mask], ref[k][mask], *[np.broadcast_to(x, g.shape)[mask] for x in ins]))
    print("refine_step %s: worst latent / moment error %.2f ulp" % (name, worst))
    assert worst <= 16.0


def crafted_trace(B=6):
    """n = 0 everywhere: J = -rec exactly.  Per image the J of iterations 0, 1, 2 (see tests/test_refine_host.py::test_keep_rule_rows)"""
    rec = np.array([[np.nan, 5.0, 5.0, np.nan, np.inf, np.inf], [3.0, np.nan, 5.0, np.nan, np.inf, 7.0], [4.0, 4.0, 4.0, np.nan, 9.0, np.inf]],
                   np.float32)
    return rec[:, :B]


@pytest.mark.parametrize("A,G", [(8, 12), (7, 9)])
def test_keep_rule_is_bit_exact_on_crafted_traces(gpu_device, A, G):
    from attend_infer_repeat_amd import refine
    T, B = 2, 6
    rec = crafted_trace(B)
    best_dev, best_ref = None, None
    for it in range(3):
        case = step_case(T, B, A, G, seed=it, n=[0] * B, n_bands=1)
        case["rec_parts"] = rec[it:it + 1].copy()
        ref = refine.reference_step(**case, priors=(0, 1, 0, 1, 0, 1), lr_what=0.0, lr_where=0.0, **ADAM, c1=0.1, c2=0.001, guard_eps=0.0,
                                    iter=it, do_update=0, best=best_ref)
        got, st = run_step(case, (0, 1, 0, 1, 0, 1), 0.0, 0.0, 0.1, 0.001, 0.0, it, 0, best=best_dev, trace_rows=3)
        assert st == 0
        best_ref = ref["best"]
        best_dev = {k: got[k] for k in ("best_J", "best_iter", "best_what", "best_where", "best_glimpse", "J_trace")}
        assert np.array_equal(got["best_J"].cpu().numpy(), best_ref["J"], equal_nan=True), it
        assert np.array_equal(got["best_iter"].cpu().numpy(), best_ref["iter"]), it
        for k in ("what", "where", "glimpse"):
            assert np.array_equal(got["best_" + k].cpu().numpy(), best_ref[k].astype(np.float32)), (it, k)
        for k in MOVING:                                           # do_update = 0: nothing moves
            assert np.array_equal(got[k].cpu().numpy(), case[k]), k
    assert best_ref["iter"].tolist() == [1, 2, 2, 0, 2, 1]          # NaN never replaces; ties keep the earlier; -inf is a value
    assert np.array_equal(got["J_trace"].cpu().numpy(), -rec, equal_nan=True)


def test_learning_rate_zero_and_the_guard_rule(gpu_device):
    T, B, A, G = 3, 5, 7, 9
    priors = (0.0, 1.0, 1.0, 0.5, 0.0, 1.0)
    case = step_case(T, B, A, G, seed=9, n=[3, 3, 2, 1, 0])
    case["where"][0, 0] = [0.0, 0.3, -1e-4, 0.2]                   # sx = 0 -> +guard; a tiny negative sy keeps its sign
    case["where"][1, 0] = [-0.0, 0.3, 0.01, 0.2]
    case["dwhere"][:2, 0] = 0.0
    case["m_where"][:2, 0] = 0.0
    mask = case["presence"] > 0.5
    c1, c2 = 0.1, 0.001
    for lr in ((0.0, 1e-2), (1e-2, 0.0)):
        got, st = run_step(case, priors, lr[0], lr[1], c1, c2, 0.05, 0, 1)
        assert st == 0
        still, moved = ("what", "where") if lr[0] == 0.0 else ("where", "what")
        assert np.array_equal(got[still].cpu().numpy(), case[still])                      # not even the guard rule touches it
        assert (got[moved].cpu().numpy()[mask] != case[moved][mask]).any()
        for k in ("m_what", "v_what", "m_where", "v_where"):       # the moments move either way
            assert (got[k].cpu().numpy()[mask] != case[k][mask]).all(), k
    # the guard: lr tiny, so every guarded component lands on +-guard or stays (almost) where it was
    got, st = run_step(case, priors, 1e-2, 1e-7, c1, c2, 0.05, 0, 1)
    w = got["where"].cpu().numpy()
    assert w[0, 0, 0] == np.float32(0.05) and w[0, 0, 2] == np.float32(-0.05) and w[1, 0, 2] == np.float32(0.05)
    assert abs(w[1, 0, 0]) == np.float32(0.05)
    assert np.array_equal(w[0, 0, 1::2] != 0.05, [True, True]) and (np.abs(w[..., 0::2][mask]) >= np.float32(0.05)).all()
    big = mask[..., None] & (np.abs(case["where"]) >= 0.06)
    assert np.allclose(w[big], case["where"][big], atol=1e-5)
    off, _ = run_step(case, priors, 1e-2, 1e-7, c1, c2, 0.0, 0, 1)
    assert abs(off["where"][0, 0, 0].item()) < 1e-5                # without the guard the zero stays (nearly) a zero


def test_argument_checks_return_their_code_and_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    T, B, A, G = 3, 5, 8, 12
    priors = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    case = step_case(T, B, A, G, seed=1)

    def call(expect, iter=0, do_update=1, drop=(), shapes=None, misalign=(), priors=priors):
        d = {k: torch.from_numpy(v).cuda() for k, v in case.items()}
        outs = dict(best_J=torch.full((B,), SENTINEL_F, dtype=torch.float64).cuda(), best_iter=torch.full((B,), SENTINEL_I,
                                                                                                         dtype=torch.int32).cuda(),
                    best_what=torch.full((T, B, A), SENTINEL_F).cuda(), best_where=torch.full((T * B * 4 + 4,), SENTINEL_F).cuda(),
                    best_glimpse=torch.full((T, B, G), SENTINEL_F).cuda(), J_trace=torch.full((2, B), SENTINEL_F).cuda())
        d.update(outs)
        d["where"] = torch.cat([d["where"].reshape(-1), torch.zeros(4).cuda()])             # room to shift the pointer by one float
        before = {k: v.clone() for k, v in d.items()}
        ptr = {k: (None if k in drop else Hh._p(v.reshape(-1)[1:] if k in misalign else v)) for k, v in d.items()}
        t, b, a, g = shapes or (T, B, A, G)
        st = Hh.lib().air_refine_step(ptr["what"], ptr["where"], ptr["glimpse"], ptr["presence"], ptr["rec_parts"], 3, ptr["dwhat"],
                                      ptr["dwhere"], ptr["where_loc"], *priors, ptr["m_what"], ptr["v_what"], ptr["m_where"],
                                      ptr["v_where"], 1e-2, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.001, 0.0, iter, do_update, t, b, a, g,
                                      ptr["best_J"], ptr["best_iter"], ptr["best_what"], ptr["best_where"], ptr["best_glimpse"],
                                      ptr["J_trace"], Hh._stream())
        torch.cuda.synchronize()
        assert st == expect, (st, expect)
        for k in d:
            assert same_bits(d[k], before[k]), k

    for k in ("what", "where", "glimpse", "presence", "rec_parts", "best_J", "best_iter", "best_what", "best_where", "best_glimpse",
              "dwhat", "dwhere", "m_what", "v_what", "m_where", "v_where"):
        call(-1, drop=(k,))                                        # AIR_E_NULL
    for shapes in ((0, B, A, G), (33, B, A, G), (T, 0, A, G), (T, B, 0, G), (T, B, A, 0), (T, -1, A, G)):
        call(-2, shapes=shapes)                                    # AIR_E_SHAPE
    call(-2, iter=-1)
    call(-1, drop=("where_loc",), priors=(0.0, 1.0, 0.0, 1.0, float("nan"), 1.0))        # a centred shift prior needs where_loc
    for k in ("where", "best_where", "dwhere", "where_loc", "m_where", "v_where"):
        call(-3, misalign=(k,))                                    # AIR_E_ALIGN


@pytest.mark.parametrize("A,G", [(8, 12), (7, 9)])
def test_the_trace_is_optional(gpu_device, A, G):
    """J_trace = NULL: every other output has the bits of the call with a trace, and where_loc = NULL is accepted with a given shift
    loc"""
    T, B = 3, 5
    priors = (0.1, 1.5, 1.0, 0.5, 0.25, 2.0)
    case = step_case(T, B, A, G, seed=4)
    c1, c2 = F32(1 - 0.9), F32(1 - 0.999)
    a, st_a = run_step(case, priors, F32(1e-2), F32(3e-2), c1, c2, 0.0, 0, 1)
    b, st_b = run_step(case, priors, F32(1e-2), F32(3e-2), c1, c2, 0.0, 0, 1, no_trace=True)
    assert st_a == 0 and st_b == 0
    assert (b["J_trace"] == SENTINEL_F).all() and same_bits(a["J_trace"][0].double(), a["best_J"].float().double())
    for k in MOVING + ("best_J", "best_iter", "best_what", "best_where", "best_glimpse"):
        assert same_bits(a[k], b[k]), k
    assert (b["best_iter"] == 0).all() and not (b["best_what"] == SENTINEL_F).any()


# ---- 2. ParseRefiner behind a parser ------------------------------------------------------------------------------------------------
def make_refiner(name, steps, lr=(1e-2, 1e-2), eps=1e-8, particles=None, capture=False, **cfg_kw):
    from attend_infer_repeat_amd.refine import ParseRefiner
    ocfg, B, params, obs = e2e_case(name)
    if cfg_kw:
        ocfg = dataclasses.replace(ocfg, **cfg_kw)
    if particles is None:
        ps = make_parser(ocfg, B, params)
    else:
        from attend_infer_repeat_amd.particle_parse import ParticleParser
        ps = ParticleParser(engine_config(ocfg), B, particles, seed=1, mask_threshold=MASK_THRESHOLD)
        ps.load_parameters(params)
        ps.set_global_step(20000)
    rf = ParseRefiner(ps, steps, lr[0], lr[1], eps=eps)
    if capture:
        ps.capture()
        rf.capture()
    return rf, ocfg, B, params, obs


def mixed_counts(ocfg, B):
    """given counts b mod (T + 1): every count from 0 to T occurs, whatever the untrained count head says"""
    return (torch.arange(B) % (ocfg.max_steps + 1)).to(torch.int32).cuda()


def f64_objective(ocfg, params, what, where, presence, obs, where_loc):
    """(J [B], rec [B]) in float64 through the oracle's decoder (mlp), canvas write (st_write) and reconstruction term; torch, so that
    autograd gives the gradients"""
    T, B, A = what.shape
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    p64 = f64(params)
    glimpse = O.mlp(what.reshape(T * B, A), p64, "glimpse_decoder", len(ocfg.glimpse_decoder_hidden) + 1, True).reshape(T, B, h, w)
    canvas = sum(presence[t][:, None, None] * O.st_write(glimpse[t], where[t], (H, W)) for t in range(T))
    z = (obs.double().reshape(B, H, W) - ocfg.output_multiplier * canvas) / ocfg.output_std
    rec = (0.5 * z * z + 0.5 * math.log(2 * math.pi) + math.log(ocfg.output_std)).reshape(B, -1).sum(1)
    N = torch.distributions.Normal
    one = torch.ones((), dtype=torch.float64)
    lp = N(ocfg.what_prior[0] * one, ocfg.what_prior[1] * one).log_prob(what).sum(-1)
    sl = ocfg.where_shift_prior[0]
    for j in range(4):
        if j % 2 == 0:
            lp = lp + N(ocfg.where_scale_prior[0] * one, ocfg.where_scale_prior[1] * one).log_prob(where[..., j])
        else:
            lp = lp + N(where_loc[..., j] if sl is None else sl * one, ocfg.where_shift_prior[1] * one).log_prob(where[..., j])
    return -rec + (presence * lp).sum(0), rec, glimpse


def f64_loop(ocfg, params, start, obs, steps, lr, eps):
    """the float64 trajectory: refine.reference_step driven by autograd gradients of sum_b rec_b.  Returns the list of per-iteration
    dicts (J, what, where BEFORE the update of that iteration, g_what, g_where = the full gradient of -J), and the final `best`."""
    from attend_infer_repeat_amd import refine
    what, where = start["what"].double().numpy(), start["where"].double().numpy()
    presence, where_loc = start["presence"].double(), start["where_loc"].double()
    T, B, A = what.shape
    zeros = lambda a: np.zeros_like(a)
    m = dict(m_what=zeros(what), v_what=zeros(what), m_where=zeros(where), v_where=zeros(where))
    priors = (*ocfg.what_prior, *ocfg.where_scale_prior, *ocfg.where_shift_prior)
    best, trace = None, []
    for i in range(steps + 1):
        wt, wh = torch.from_numpy(what).requires_grad_(True), torch.from_numpy(where).requires_grad_(True)
        J, rec, glimpse = f64_objective(ocfg, params, wt, wh, presence, obs, where_loc)
        d_what, d_where = torch.autograd.grad(rec.sum(), (wt, wh), retain_graph=True)
        g_what, g_where = torch.autograd.grad(-J.sum(), (wt, wh))
        trace.append(dict(J=J.detach().numpy(), what=what, where=where, d_what=d_what.numpy(), d_where=d_where.numpy(),
                          g_what=g_what.numpy(), g_where=g_where.numpy()))
        out = refine.reference_step(what, where, glimpse.detach().reshape(T, B, -1).numpy(), presence.numpy(), rec.detach().numpy()[None],
                                    d_what.numpy(), d_where.numpy(), where_loc.numpy(), priors, **m, lr_what=F32(lr[0]), lr_where=F32(lr[1]),
                                    beta1=F32(0.9), beta2=F32(0.999), eps=F32(eps), c1=F32(1 - 0.9 ** (i + 1)),
                                    c2=F32(1 - 0.999 ** (i + 1)),
                                    guard_eps=ocfg.guard_eps, iter=i, do_update=int(i < steps), best=best)
        assert np.allclose(out["J"], trace[-1]["J"], rtol=1e-12, atol=1e-9, equal_nan=True)      # the two restatements of J agree
        best = out["best"]
        what, where = out["what"], out["where"]
        m = {k: out[k] for k in m}
    return trace, best


def start_of(rf, out):
    """the start parse (host tensors): the bound parser's rows, its presence chain, and the where_loc the refiner centres on"""
    st = rf._start
    return dict(what=st["what"].detach().cpu().clone(), where=st["where"].detach().cpu().clone(),
                presence=rf.parser.presence.detach().cpu().clone(), where_loc=rf.where_loc.detach().cpu().clone())


GRAD_CASES = [("tiny", {}), ("t1_b5", {}), ("rect_t5", {}), ("rect_t5", dict(where_shift_prior=(None, 1.0)))]


@pytest.mark.parametrize("name,cfg_kw", GRAD_CASES)
def test_gradients_match_f64_autograd_at_the_start_latents(gpu_device, name, cfg_kw):
    rf, ocfg, B, params, obs = make_refiner(name, 1, **cfg_kw)
    out = rf.parse(obs.cuda(), mixed_counts(ocfg, B))
    rf.synchronize()
    start = start_of(rf, out)
    trace, _ = f64_loop(ocfg, params, start, obs, 0, (0.0, 0.0), 1e-8)
    label = name + ("_centred" if cfg_kw else "")
    n = start["presence"].sum(0)
    assert n.tolist() == mixed_counts(ocfg, B).tolist()
    check_tensor("refine_grad", label, "grad", "grad_what", out["grad_what"], torch.from_numpy(trace[0]["d_what"]), GRAD_TOL, GRAD_L2)
    check_tensor("refine_grad", label, "grad", "grad_where", out["grad_where"], torch.from_numpy(trace[0]["d_where"]), GRAD_TOL, GRAD_L2)
    absent = start["presence"] < 0.5
    assert (out["grad_what"].cpu()[absent] == 0).all() and (out["grad_where"].cpu()[absent] == 0).all()
    check_tensor("refine_grad", label, "out", "objective_start", out["objective_start"], torch.from_numpy(trace[0]["J"]), OUT_TOL, OUT_L2)


@pytest.mark.parametrize("name", ["rect_t5", "mnist_b8"])
def test_gradients_behind_a_particle_parser_with_a_centred_shift_prior(gpu_device, name):
    """the one configuration in which a copy runs outside the refiner's launch list: particle 0's where_loc rows are gathered before
    the list (the particles of an image share where_loc), and the kept particle's sampled latents are the start"""
    K = 4
    rf, ocfg, B, params, obs = make_refiner(name, 1, particles=K, where_shift_prior=(None, 1.0))
    out = rf.parse(obs.cuda())
    rf.synchronize()
    loc = rf.engine.where_loc.view(rf.T, B, K, 4)
    assert torch.equal(rf.where_loc, loc[:, :, 0]) and torch.equal(loc, loc[:, :, :1].expand_as(loc))
    start = start_of(rf, out)
    assert torch.equal(start["what"], rf.parser.what_sel.cpu()) and not torch.equal(start["where"], start["where_loc"])
    n = start["presence"].sum(0)
    print("refine_grad %s behind ParticleParser(K=%d): counts %s" % (name, K, n.tolist()))
    assert n.max() > 0                                             # (the sampled chains of these seeds keep objects)
    trace, _ = f64_loop(ocfg, params, start, obs, 0, (0.0, 0.0), 1e-8)
    label = name + "_particles_centred"
    check_tensor("refine_grad", label, "grad", "grad_what", out["grad_what"], torch.from_numpy(trace[0]["d_what"]), GRAD_TOL, GRAD_L2)
    check_tensor("refine_grad", label, "grad", "grad_where", out["grad_where"], torch.from_numpy(trace[0]["d_where"]), GRAD_TOL, GRAD_L2)
    check_tensor("refine_grad", label, "out", "objective_start", out["objective_start"], torch.from_numpy(trace[0]["J"]), OUT_TOL, OUT_L2)
    # the centring is seen: the same start under a prior centred elsewhere has another objective wherever an object is present
    other, _ = f64_loop(dataclasses.replace(ocfg, where_shift_prior=(0.0, 1.0)), params, start, obs, 0, (0.0, 0.0), 1e-8)
    assert ((trace[0]["J"] != other[0]["J"]) == (n.numpy() > 0)).all()


TRAJ_STEPS, TRAJ_LR, TRAJ_EPS = 4, (1e-2, 1e-2), 1.0


@pytest.fixture(scope="module")
def trajectories():
    """per case: the device result of a steps = 4, eps = 1, lr = 1e-2 call and the float64 loop from the same start (computed once)"""
    cache = {}

    def get(name):
        if name not in cache:
            rf, ocfg, B, params, obs = make_refiner(name, TRAJ_STEPS, TRAJ_LR, TRAJ_EPS)
            out = {k: v.detach().cpu().clone() for k, v in rf.parse(obs.cuda(), mixed_counts(ocfg, B)).items()}
            rf.synchronize()
            start = start_of(rf, out)
            trace, best = f64_loop(ocfg, params, start, obs, TRAJ_STEPS, TRAJ_LR, TRAJ_EPS)
            cache[name] = dict(rf=rf, ocfg=ocfg, B=B, params=params, obs=obs, out=out, start=start, trace=trace, best=best,
                               last=dict(what=rf.what.cpu().clone(), where=rf.where.cpu().clone()))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["tiny", "t1_b5", "rect_t5", "mnist_b8"])
def test_trajectory_matches_the_f64_loop(gpu_device, trajectories, name):
    """Worst observed on an MI355X, as the share of the bar used by (what, where, objective_trace): tiny (4e-4, 1e-4, 2e-4) of
    bar_z = 4.38e-4 / bar_J = 0.029; t1_b5 (4e-4, 3e-4, 5e-4) of 1.83e-4 / 0.0072; rect_t5 and mnist_b8 below 5e-5 of 2.1e-2 / 57 and
    2.3e-2 / 54 (max|g| 9.1, 3.8, 432, 477).  The device is a few fp32 roundings from the float64 loop: the gradient error the bar
    allows for is not used up."""
    c = trajectories(name)
    trace, out = c["trace"], c["out"]
    gmax = max(max(np.abs(t["g_what"]).max(), np.abs(t["g_where"]).max()) for t in trace)
    bar_z = 4 * TRAJ_STEPS * TRAJ_LR[0] * GRAD_TOL * gmax
    present = c["start"]["presence"].numpy() > 0.5
    used = {}
    for k in ("what", "where"):
        err = np.abs(c["last"][k].double().numpy() - trace[-1][k])
        assert np.array_equal(c["last"][k].numpy()[~present], c["start"][k].numpy()[~present]), k     # absent rows never move
        used[k] = float(err.max() / bar_z) if bar_z > 0 else 0.0
    Jref = np.stack([t["J"] for t in trace])
    l1 = max((np.abs(t["g_what"]).sum((0, 2)) + np.abs(t["g_where"]).sum((0, 2))).max() for t in trace)
    bar_J = OUT_TOL * np.abs(Jref).max() + l1 * bar_z
    used["objective_trace"] = float(np.abs(out["objective_trace"].double().numpy() - Jref).max() / bar_J)
    print("refine trajectory %s: max|g| %.3g, bar_z %.3g, bar_J %.3g, share of the bar used %s"
          % (name, gmax, bar_z, bar_J, {k: round(v, 4) for k, v in used.items()}))
    assert all(v <= 1.0 for v in used.values()), used
    # improvement: wherever the float64 loop gains more than twice the J bar, the device's best beats its start
    gain = c["best"]["J"] - Jref[0]
    sure = gain > 2 * OUT_TOL * np.abs(Jref).max()
    obj, obj0 = out["objective"].numpy(), out["objective_start"].double().numpy()
    print("refine trajectory %s: float64 gain %s, device gain %s" % (name, np.round(gain, 4).tolist(), np.round(obj - obj0, 4).tolist()))
    assert (obj[sure] > obj0[sure]).all()


@pytest.mark.parametrize("name", ["tiny", "rect_t5"])
def test_best_is_monotone_and_a_bit_copy_of_its_iteration(gpu_device, trajectories, name):
    from attend_infer_repeat_amd.refine import ParseRefiner
    c = trajectories(name)
    out, rf, B = c["out"], c["rf"], c["B"]
    obj, obj0, it = out["objective"], out["objective_start"], out["best_iter"].long()
    ok = ~torch.isnan(obj0)
    assert (obj.float()[ok] >= obj0[ok]).all()
    assert same_bits(obj.float(), out["objective_trace"][it, torch.arange(B)])
    assert same_bits(out["objective_start"], out["objective_trace"][0])
    # nothing in the trace beats the kept iteration (rounding to fp32 is monotone), and nothing before it ties it in float64 terms
    tr = torch.where(torch.isnan(out["objective_trace"]), torch.full_like(out["objective_trace"], -float("inf")), out["objective_trace"])
    assert (ok.logical_not() | (tr[it, torch.arange(B)] >= tr.max(0).values)).all()
    # the returned rows are the iterate of iteration best_iter: run exactly that many steps and look at the live latents
    for k in sorted(set(it.tolist())):
        again = ParseRefiner(rf.parser, k, TRAJ_LR[0], TRAJ_LR[1], eps=TRAJ_EPS)
        o2 = again.parse(c["obs"].cuda(), mixed_counts(c["ocfg"], B))
        again.synchronize()
        sel = (it == k).nonzero().reshape(-1)
        glimpse_k = (again._start["glimpse"] if k == 0 else again.act[-1]).reshape(rf.T, B, -1).cpu()
        assert torch.equal(out["what"][:, sel], again.what.cpu()[:, sel]), k
        assert torch.equal(out["where"][:, sel], again.where.cpu()[:, sel]), k
        assert torch.equal(out["glimpse"].reshape(rf.T, B, -1)[:, sel], glimpse_k[:, sel]), k
        assert same_bits(out["objective_trace"][k, sel], o2["objective_trace"].cpu()[k, sel]), k


BIT_KEYS_OFF = ("layers",)


@pytest.mark.parametrize("name,particles", [("tiny", None), ("rect_t5", None), ("t1_b5", None), ("tiny", 4), ("mnist_b8", 4)])
def test_zero_steps_is_the_bound_parser_bit_for_bit(gpu_device, name, particles):
    rf, ocfg, B, params, obs = make_refiner(name, 0, particles=particles)
    kw = {} if particles is None else dict(sample_noise=False)
    if particles is not None:
        rf.parser.parse(obs.cuda())                                # draw noise once; the calls below keep it
    base = {k: v.detach().clone() for k, v in rf.parser.parse(obs.cuda(), **kw).items()}
    out = rf.parse(obs.cuda(), **kw)
    rf.synchronize()
    assert set(base) - set(BIT_KEYS_OFF) <= set(out)
    for k in base:
        if k not in BIT_KEYS_OFF:
            assert same_bits(out[k], base[k].reshape(out[k].shape)), k
    assert set(out) - set(base) == {"objective", "objective_start", "best_iter", "objective_trace", "grad_what", "grad_where"}
    assert (out["best_iter"] == 0).all() and tuple(out["objective_trace"].shape) == (1, B)
    assert same_bits(out["objective"].float(), out["objective_start"])
    assert rf.launch_count()["decoder_fwd"] == 0 and rf.launch_count()["refine_step"] == 1


@pytest.mark.parametrize("name,particles", [("mnist_b8", None), ("rect_t5", 4)])
def test_graph_replay_equals_eager(gpu_device, name, particles):
    eager, ocfg, B, params, _ = make_refiner(name, 3, particles=particles)
    graph = make_refiner(name, 3, particles=particles, capture=True)[0]
    kw = {} if particles is None else dict(sample_noise=False)
    args = (mixed_counts(ocfg, B),) if particles is None else ()   # (the untrained count head of mnist_b8 says n = 0 everywhere)
    noise = O.make_noise(ocfg, B * (particles or 1), seed=5)
    for rf in (eager, graph):
        if particles is not None:
            rf.engine.set_noise(noise["eps_where"].cuda(), noise["eps_what"].cuda(), noise["u_pres"].cuda())
    kept = []
    for seed in (11, 12):
        obs = O.synthetic_batch(ocfg, B, seed=seed)[0].cuda()
        a, b = eager.parse(obs, *args, **kw), graph.parse(obs, *args, **kw)
        eager.synchronize(); graph.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
        kept.append(b["objective_trace"].clone())
    assert not same_bits(kept[0], kept[1])
    n = graph.launch_count()
    L = len(ocfg.glimpse_decoder_hidden) + 1
    assert {k: v for k, v in n.items() if k != "parser"} == {"start": 3, "decoder_fwd": 4 * L, "canvas_fwd": 4, "canvas_bwd": 3,
                                                             "decoder_dx": 3 * L, "refine_step": 4, "parse_objects": 1,
                                                             "parse_render": 1, "rec_sum": 1}
    assert n["parser"] == graph.parser.launch_count()
    # update_config re-captures: a changed output_multiplier changes the objective, and changing it back restores the bits
    assert graph.update_config(output_multiplier=0.25) and graph._graph is not None
    c = graph.parse(obs, *args, **kw)["objective_trace"].clone()
    assert not same_bits(c, kept[1])
    assert graph.update_config(output_multiplier=float(ocfg.output_multiplier))
    assert same_bits(graph.parse(obs, *args, **kw)["objective_trace"], kept[1])
    graph.release_graphs(); graph.parser.release_graphs()


def test_scorer_bound_to_a_refiner_scores_the_refined_parse(gpu_device):
    from attend_infer_repeat_amd.score import ParseScorer
    from test_score import annotated_batches
    rf, ocfg, B, params, _ = make_refiner("mnist_b8", 2)
    T, G = ocfg.max_steps, 2
    fake = types.SimpleNamespace(engine=rf.engine, T=rf.T, R=rf.R, **{k: torch.zeros_like(getattr(rf, k)) for k in
                                                                     ("owner", "boxes", "num_objects", "score", "presence")})
    sc, sc_hand = ParseScorer(rf, G, max_batches=4), ParseScorer(fake, G, max_batches=4)
    for i, b in enumerate(annotated_batches("mnist_b8", B, 2, seed=3)):
        out = rf.parse(torch.from_numpy(b["obs"]).cuda())
        for k in ("owner", "boxes", "num_objects", "score", "presence"):
            assert out[k].data_ptr() == getattr(rf, k).data_ptr()
            getattr(fake, k).copy_(out[k])
        sc.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
        sc_hand.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
    a, h = sc.summary(), sc_hand.summary()
    assert set(a) == set(h) and a["images"] == 2 * B
    for k in a:
        assert a[k] == h[k] or (math.isnan(a[k]) and math.isnan(h[k])), k


# ---- 3. the model and the surface ---------------------------------------------------------------------------------------------------
def test_refinement_on_the_model_does_not_disturb_training(gpu_device):
    B, T, A = 8, 3, 50
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    before = _train_state(air._engine)
    plain = {k: v.clone() for k, v in air.parse().items()}
    out = air.parse(refine=3, refine_lr=(1e-2, 1e-3))
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert out is air.parsed and set(out) - set(plain) == {"objective", "objective_start", "best_iter", "objective_trace", "grad_what",
                                                           "grad_where"}
    assert {k: tuple(out[k].shape) for k in set(out) - set(plain)} == {
        "objective": (B,), "objective_start": (B,), "best_iter": (B,), "objective_trace": (4, B), "grad_what": (T, B, A),
        "grad_where": (T, B, 4)}
    assert out["objective"].dtype == torch.float64 and out["best_iter"].dtype == torch.int32
    for k in ("num_objects", "presence", "presence_prob", "num_steps_posterior", "score", "count_prob"):     # the count does not move
        assert torch.equal(out[k], plain[k]), k
    assert (out["objective"].float() >= out["objective_start"]).all() and torch.isfinite(out["reconstruction"]).all()
    # cached per (batch, particles, select, N, lr); refine=None is the old path, bit for bit
    r = air._parse_refiners
    assert len(r) == 1 and air.parse(refine=3, refine_lr=(1e-2, 1e-3)) is air.parsed and len(air._parse_refiners) == 1
    air.parse(refine=0)
    assert len(air._parse_refiners) == 2
    again = air.parse()
    assert set(again) == set(plain) and all(torch.equal(again[k], plain[k]) for k in plain)
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # the loggers against a torch recomputation
    from attend_infer_repeat_amd.evaluation import make_parse_logger
    got = make_parse_logger(air, lambda: (x, y), 2, "test", refine=3, refine_lr=(1e-2, 1e-3))(itr=3)
    assert set(got) == {"map_num_step_acc", "count_prob", "num_objects", "objective_gain", "refine_moved"}
    o = air.parse(x, refine=3, refine_lr=(1e-2, 1e-3))
    gain = (o["objective"] - o["objective_start"].double())
    assert abs(got["objective_gain"] - gain.mean().item()) <= 1e-9 * (1 + abs(gain.mean().item()))
    assert got["refine_moved"] == (o["best_iter"] > 0).double().mean().item()
    got_p = make_parse_logger(air, lambda: (x, y), 1, "test", particles=2, refine=1)(itr=3)
    assert {"objective_gain", "refine_moved", "best_particle_moved", "ess"} <= set(got_p)


def test_score_parse_with_refinement_and_the_score_logger(gpu_device):
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.evaluation import make_parse_score_logger
    B = 8
    air, ts, x, y = _mnist_air(B)
    d = procedural_multi_mnist(B, seed=3, n_templates=200, return_annotations=True)
    data = dict(imgs=d["imgs"].astype(np.float32) / 255.0, instances=d["instances"], boxes=d["boxes"])
    air.score_parse(torch.from_numpy(data["imgs"]).cuda(), data["instances"], data["boxes"], accumulate=False, refine=2)
    sc = air.parse_scorer(2, refine=2)
    assert sc.parser is air._parser_for(None, "joint", 2, None) and sc.parser.steps == 2
    s = sc.summary()
    assert s["images"] == B
    # by hand: the refiner's owner / boxes through the plain scorer's kernels give the same summary
    from attend_infer_repeat_amd.score import ParseScorer
    rf = sc.parser
    fake = types.SimpleNamespace(engine=rf.engine, T=rf.T, R=rf.R, **{k: getattr(rf, k).clone() for k in
                                                                     ("owner", "boxes", "num_objects", "score", "presence")})
    hand = ParseScorer(fake, 2)
    hand.score(data["instances"], data["boxes"], accumulate=False)
    h = hand.summary()
    for k in s:
        assert s[k] == h[k] or (math.isnan(s[k]) and math.isnan(h[k])), k
    got = make_parse_score_logger(air, data, 1, "test", refine=2)(itr=1)
    assert {"objective_gain", "refine_moved", "count_acc", "map", "fg_ari"} <= set(got)


def test_training_script_parse_refine_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--parse-eval",
                            "--parse-refine", "2", "--parse-refine-lr", "0.01,0.001"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse+refine(2) ") == 2
    for l in rec:
        assert l["refine"] == 2 and l["refine_lr"] == [0.01, 0.001] and 0.0 <= l["refine_moved"] <= 1.0 and l["objective_gain"] >= 0.0
    with pytest.raises(SystemExit):
        multi_mnist.main(["--parse-refine-lr", "0.1,0.1"])
    with pytest.raises(SystemExit):
        multi_mnist.main(["--parse-refine", "2", "--parse-refine-lr", "0.1"])
