"""GPU tests of the K-particle importance-weighted evaluation (attend_infer_repeat_amd/iw_eval.py, csrc/iw_kernels.hip):
log-weights against the float64 oracle, the reduce kernel against float64 on its own input, the weights against the
training loss's KL rows, graph replay / running totals, and the public surface (AIRonMNIST.evaluate_iw, make_iw_logger,
scripts/multi_mnist.py --iw-particles).

Bars.  log w is a sum of per-sample outputs the engine suite already pins (dominated by rec_loss_per_sample), so test 1 uses
that suite's per-sample output bars OUT_TOL = 1e-4 (worst element / tensor max) and OUT_L2 = 3e-5 (relative L2); the float32
oracle sits at <= 2.4e-6 / 3.6e-7 from the float64 oracle on these cases.  The reduce kernel sees the SAME fp32 inputs as its
float64 reference (only fp32 exp and summation differ): the project's scalar bar 2e-5 * (|ref| + 1)."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import air_oracle as O
from test_engine import CONFIGS, OUT_L2, OUT_TOL, _separate_borderline_draws, check_tensor, f64, rel_err

pytestmark = pytest.mark.gpu

GSTEP = 20000
CASES = {
    "tiny_b6_k5": (CONFIGS["tiny"][0], 6, 5),
    "mnist_b8_k8": (O.AIRConfig(), 8, 8),                         # latency plan
    "rect_t5_b3_k4": (CONFIGS["rect_t5"][0], 3, 4),
    "mnist_b16_k64": (O.AIRConfig(), 16, 64),                     # 1024 rows, 3072 glimpses: the throughput plan
}


def engine_config(ocfg, mfma_dtype="f32"):
    from attend_infer_repeat_amd.engine_config import EngineConfig
    fields = {f.name for f in dataclasses.fields(EngineConfig)}
    return EngineConfig(mfma_dtype=mfma_dtype, **{k: v for k, v in dataclasses.asdict(ocfg).items() if k in fields})


def make_inputs(ocfg, B, K):
    """parameters, images and noise as tests/test_engine.py::make_pair draws them, the noise for K * B rows"""
    params = O.init_params(ocfg, seed=1, bias_std=0.1)
    obs, _ = O.synthetic_batch(ocfg, B, seed=11)
    noise = O.make_noise(ocfg, K * B, seed=21)
    return params, obs, noise


def make_evaluator(ocfg, B, K, params, noise, normalize=True, mfma_dtype="f32", seed=0):
    from attend_infer_repeat_amd.iw_eval import ImportanceEvaluator
    ev = ImportanceEvaluator(engine_config(ocfg, mfma_dtype), B, K, seed=seed, normalize_steps_prior=normalize)
    ev.load_parameters(params)
    if noise is not None:
        ev.engine.set_noise(noise["eps_where"].cuda(), noise["eps_what"].cuda(), noise["u_pres"].cuda())
    ev.set_global_step(GSTEP)
    return ev


def oracle_log_weights(ocfg, params, obs, noise, K, normalize, gstep=GSTEP):
    """log w [R] and n [R] (R = K * B, row b * K + k) in float64 from the oracle's outputs on the K-tiled images; also the outputs"""
    tiled = obs.repeat_interleave(K, 0)
    res = O.objective(f64(params), ocfg, tiled.double(), f64(noise), global_step=gstep)
    T, R = ocfg.max_steps, tiled.shape[0]
    N = torch.distributions.Normal
    z = res["presence"].reshape(T, R)
    n = z.sum(0)
    one = torch.ones((), dtype=torch.float64)
    lr_what = (N(ocfg.what_prior[0] * one, ocfg.what_prior[1] * one).log_prob(res["what"])
               - N(res["what_loc"], res["what_scale"]).log_prob(res["what"])).sum(-1)
    wl = res["where_loc"]
    shift_loc = wl[..., 1::2] if ocfg.where_shift_prior[0] is None else ocfg.where_shift_prior[0] * torch.ones_like(wl[..., 1::2])
    p_loc = torch.stack([ocfg.where_scale_prior[0] * torch.ones_like(wl[..., 0]), shift_loc[..., 0],
                         ocfg.where_scale_prior[0] * torch.ones_like(wl[..., 0]), shift_loc[..., 1]], -1)
    p_scale = torch.tensor([ocfg.where_scale_prior[1], ocfg.where_shift_prior[1]] * 2, dtype=torch.float64)
    lr_where = (N(p_loc, p_scale).log_prob(res["where"]) - N(wl, res["where_scale"]).log_prob(res["where"])).sum(-1)
    prior = O.geometric_prior(O.steps_prior_success_prob(ocfg, gstep), T)
    if normalize:
        prior = prior / prior.sum()
    log_pi = torch.log(prior)[n.long()]
    log_qn = O.num_steps_log_prob(res["num_steps_posterior"].double(), n)
    logw = -res["rec_loss_per_sample"] + log_pi - log_qn + (z * (lr_what + lr_where)).sum(0)
    return logw, n, res


def f64_reduce(logw, n, T):
    """iw_bound, elbo, ess, q_n_iw of [B, K] log-weights in torch float64"""
    lw = logw.detach().cpu().double()
    nn = n.detach().cpu().long()
    K = lw.shape[1]
    wn = torch.softmax(lw, 1)
    q = torch.stack([(wn * (nn == c)).sum(1) for c in range(T + 1)], 1)
    return dict(iw_bound=torch.logsumexp(lw, 1) - math.log(K), elbo=lw.mean(1), ess=1.0 / (wn * wn).sum(1), num_steps_posterior=q)


def check_reduce(got, ref, K):
    for k in ("iw_bound", "elbo", "ess", "num_steps_posterior"):
        g, r = got[k].detach().cpu().double(), ref[k]
        err = ((g - r).abs() / (r.abs() + 1.0)).max().item()
        print("reduce %s: worst |got - ref| / (|ref| + 1) = %.3e" % (k, err))
        assert err <= 2e-5, (k, err)
    iw, el, es = (got[k].detach().cpu().double() for k in ("iw_bound", "elbo", "ess"))
    assert (iw >= el - 2e-5 * (el.abs() + 1)).all()
    assert (es >= 1 - 2e-5 * 2).all() and (es <= K + 2e-5 * (K + 1)).all()


def run_reduce(logw, n, T):
    """air_iw_reduce alone on [B, K] device tensors"""
    from attend_infer_repeat_amd import _lib, hip as H
    B, K = logw.shape
    dev = logw.device
    out = dict(iw_bound=torch.zeros(B, device=dev), elbo=torch.zeros(B, device=dev), ess=torch.zeros(B, device=dev),
               num_steps_posterior=torch.zeros(B, T + 1, device=dev))
    torch.cuda.synchronize()
    st = H.lib().air_iw_reduce(H._p(logw), H._p(n), T, B * K, K, H._p(out["iw_bound"]), H._p(out["elbo"]), H._p(out["ess"]),
                               H._p(out["num_steps_posterior"]), None, None, None)
    _lib.check(st, "air_iw_reduce")
    torch.cuda.synchronize()
    return out


# ---- 1. log-weights against the float64 oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,normalize", [(k, True) for k in CASES] + [("tiny_b6_k5", False)])
def test_log_weights_match_f64_oracle(gpu_device, name, normalize):
    ocfg, B, K = CASES[name]
    params, obs, noise = make_inputs(ocfg, B, K)
    ev = make_evaluator(ocfg, B, K, params, noise, normalize)
    out = ev.evaluate(obs.cuda(), sample_noise=False)
    ev.synchronize()
    ref, n, res = oracle_log_weights(ocfg, params, obs, noise, K, normalize)
    T = ocfg.max_steps
    assert torch.equal(ev.engine.presence.cpu().double().reshape(T, B * K), res["presence"].reshape(T, B * K))
    assert torch.equal(out["num_steps"].cpu().reshape(-1).long(), n.long())
    counts = torch.bincount(n.long(), minlength=T + 1)
    print("particles per n:", counts.tolist(), "log w range %.1f .. %.1f" % (ref.min().item(), ref.max().item()))
    assert counts[0] > 0 and counts[T] > 0 and counts[1:T].sum() > 0, counts       # a mask error cannot hide
    assert torch.isfinite(ref).all()
    got = out["log_weights"].reshape(-1)
    print("log w: max %.3e l2 %.3e" % (rel_err(got, ref), ((got.cpu().double() - ref).norm() / ref.norm()).item()))
    check_tensor("iw_parity", "%s%s" % (name, "" if normalize else "_unnormalised"), "out", "log_weights", got, ref, OUT_TOL, OUT_L2)


# ---- 2. the reduce kernel against float64 on its own input ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mnist_b8_k8", "mnist_b16_k64"])
def test_reduce_matches_f64_on_the_kernels_log_weights(gpu_device, name):
    ocfg, B, K = CASES[name]
    params, obs, noise = make_inputs(ocfg, B, K)
    ev = make_evaluator(ocfg, B, K, params, noise)
    out = ev.evaluate(obs.cuda(), sample_noise=False)
    ev.synchronize()
    T = ocfg.max_steps
    check_reduce(out, f64_reduce(out["log_weights"], out["num_steps"], T), K)
    again = run_reduce(out["log_weights"], out["num_steps"], T)              # the entry on its own gives the same bits
    for k in again:
        assert torch.equal(again[k], out[k]), k


def test_reduce_on_synthetic_blocks(gpu_device):
    T = 3
    g = torch.Generator().manual_seed(5)
    # all equal: ess = K, iw_bound = elbo = log w
    lw = torch.full((4, 24), -37.25).cuda()
    n = torch.randint(0, T + 1, (4, 24), generator=g).int().cuda()
    out = run_reduce(lw, n, T)
    check_reduce(out, f64_reduce(lw, n, T), 24)
    assert torch.allclose(out["ess"].cpu(), torch.full((4,), 24.0), rtol=2e-5) and torch.allclose(out["iw_bound"], out["elbo"], rtol=2e-5)
    assert torch.allclose(out["iw_bound"].cpu(), torch.full((4,), -37.25), rtol=2e-5)
    # one particle 1000 nats above the rest: ess = 1 to fp32, iw_bound = max - log K
    K = 100
    lw = (torch.randn(3, K, generator=g) * 3 - 50)
    lw[torch.arange(3), torch.tensor([0, 57, 99])] += 1000.0
    n = torch.randint(0, T + 1, (3, K), generator=g).int()
    out = run_reduce(lw.cuda(), n.cuda(), T)
    check_reduce(out, f64_reduce(lw, n, T), K)
    assert torch.equal(out["ess"].cpu(), torch.ones(3))
    assert torch.allclose(out["iw_bound"].cpu().double(), lw.double().max(1).values - math.log(K), rtol=2e-5)
    best = n[torch.arange(3), torch.tensor([0, 57, 99])].long()
    assert torch.equal(out["num_steps_posterior"].cpu().argmax(1), best)
    # K = 1, and a K that is not a multiple of the wavefront
    for K in (1, 67):
        lw = torch.randn(5, K, generator=g) * 20 - 100
        n = torch.randint(0, T + 1, (5, K), generator=g).int()
        out = run_reduce(lw.cuda(), n.cuda(), T)
        check_reduce(out, f64_reduce(lw, n, T), K)
    assert torch.equal(out["num_steps_posterior"].sum(1).round().cpu(), torch.ones(5))


# ---- 3. the weights mean what the training loss means --------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,K", [("tiny", 4, 4096), ("mnist_b8", 2, 512)])
def test_log_ratio_minus_analytic_kl_has_mean_zero(gpu_device, name, B, K):
    """d_k = -log w_k - rec_k - (log q(n_k) - log pi(n_k)) - sum_t z_tk (kl_what_row_tk + kl_where_row_tk) is the sampled Gaussian
    log-ratio minus its analytic KL (the rows the engine suite pins): mean zero over the particles.  A sign, mask or prior-index error
    shifts the mean by whole nats, i.e. tens to hundreds of standard errors; the fixed seed makes the outcome deterministic (the
    oracle alone gives |mean| / se <= 1.92 and <= 1.54 on these two cases)."""
    ocfg = CONFIGS[name][0]
    params, obs, noise = make_inputs(ocfg, B, K)
    ev = make_evaluator(ocfg, B, K, params, noise, normalize=False)
    out = ev.evaluate(obs.cuda(), sample_noise=False)
    ev.synchronize()
    eng, T = ev.engine, ocfg.max_steps
    z = eng.presence.double().reshape(T, B * K)
    n = out["num_steps"].reshape(-1).long()
    log_pi = torch.log(eng.prior_dev)[n]
    kl = (z * (eng.kl_what_row.double().reshape(T, -1) + eng.kl_where_row.double().reshape(T, -1))).sum(0)
    d = -out["log_weights"].double().reshape(-1) - eng.rec.double() - (eng.logp.double() - log_pi) - kl
    d = d.reshape(B, K).cpu()
    mean, se = d.mean(1), d.std(1) / math.sqrt(K)
    print("mean", mean.tolist(), "se", se.tolist(), "|mean|/se", (mean.abs() / se).tolist())
    assert (se > 0).all() and (mean.abs() <= 5 * se).all(), (mean, se)


# ---- 4. graph and accumulators -------------------------------------------------------------------------------------------------
def _batches(ocfg, B, count):
    out = []
    for i in range(count):
        obs, _ = O.synthetic_batch(ocfg, B, seed=40 + i)
        nums = torch.from_numpy(np.random.default_rng(50 + i).integers(0, ocfg.max_steps + 1, B)).int()
        out.append((obs.cuda(), nums.cuda()))
    return out


KEYS = ("log_weights", "num_steps", "iw_bound", "elbo", "ess", "num_steps_posterior")


def test_graph_replay_equals_eager_and_totals_are_the_f64_sums(gpu_device):
    ocfg, B, K = O.AIRConfig(), 8, 8
    params, _, _ = make_inputs(ocfg, B, K)
    eager = make_evaluator(ocfg, B, K, params, None, seed=3)
    graph = make_evaluator(ocfg, B, K, params, None, seed=3)
    graph.capture()
    batches = _batches(ocfg, B, 3)
    eager.reset(); graph.reset()
    kept = []
    for obs, nums in batches:
        a = eager.evaluate(obs, nums)
        b = graph.evaluate(obs, nums)
        eager.synchronize(); graph.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k                     # same seed, same noise state: identical bits, replay == eager
        kept.append({k: b[k].clone() for k in KEYS})
    assert not torch.equal(kept[0]["log_weights"], kept[1]["log_weights"])
    # fresh particles per call: the same images again give other weights
    # (cloned on the caller's stream straight away: evaluate() orders that stream after its work)
    again = {k: v.clone() for k, v in graph.evaluate(*batches[2]).items()}
    graph.synchronize()
    assert not torch.equal(again["log_weights"], kept[2]["log_weights"])
    tot = eager.totals()
    assert tot["n_images"] == 3 * B
    for k in ("iw_bound", "elbo", "ess"):
        ref = sum(o[k].double().sum().item() for o in kept)
        assert abs(tot[k] * tot["n_images"] - ref) <= 1e-12 * abs(ref) + 1e-300, (k, tot[k], ref)
    hits = torch.cat([(o["num_steps_posterior"].argmax(1).cpu() == nums.cpu().long()) for o, (_, nums) in zip(kept, batches)])
    assert tot["num_step_acc"] == hits.double().mean().item()
    # without the true counts there is no accuracy to report
    eager.reset(); eager.evaluate(batches[0][0])
    t2 = eager.totals()
    assert t2["n_images"] == B and math.isnan(t2["num_step_acc"]) and math.isfinite(t2["iw_bound"])
    assert graph.launch_count() == {"forward": len(graph.engine._plan_fwd_noise), "rng_advance": 1, "iw": 2}


# ---- 5. through the public surface ---------------------------------------------------------------------------------------------
def _mnist_air(B=8, **kw):
    from attend_infer_repeat_amd import mnist_model, utils
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    AD = utils.AttrDict
    imgs, nums = synthetic_multi_mnist(B, (50, 50), 2, seed=0)
    x, y = torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda()
    torch.manual_seed(0)
    air = mnist_model.AIRonMNIST(x, y, max_steps=3, explore_eps=1e-3, steps_pred_hidden=[128, 64], transform_var_bias=.5,
                                 step_bias=.75, output_multiplier=.5)
    nsp = AD(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    ts, _ = air.train_step(1e-4, 0., AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp, **kw)
    return air, ts, x, y


def _train_state(eng):
    eng.synchronize()
    return {k: getattr(eng, k).clone() for k in ("flat_params", "flat_ms", "flat_mg", "flat_mom", "step_dev", "rng_state")}


def test_evaluate_iw_on_the_model_does_not_disturb_training(gpu_device):
    B = 8
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    before = _train_state(air._engine)
    assert air.evaluate_iw(particles=4) is air
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air._engine.global_step == 2 and int(air.global_step) == 2
    assert tuple(air.iw_bound_per_sample.shape) == (B,) and tuple(air.iw_num_steps_posterior.shape) == (B, 4)
    for k in ("iw_bound", "iw_elbo", "iw_ess", "iw_num_step_accuracy"):
        assert getattr(air, k).dim() == 0 and torch.isfinite(getattr(air, k)), k
    assert torch.isfinite(air.iw_bound_per_sample).all()
    assert float(air.iw_bound) >= float(air.iw_elbo) - 2e-5 * (abs(float(air.iw_elbo)) + 1) and 1 - 1e-4 <= float(air.iw_ess) <= 4 + 1e-3
    assert torch.allclose(air.iw_num_steps_posterior.sum(1), torch.ones(B, device=x.device), atol=1e-5)
    # the evaluator carries the trained weights and the training step counter
    ev = air._iw_evaluator
    assert torch.equal(ev.engine.flat_params, air._engine.flat_params) and int(ev.engine.step_dev.item()) == 2
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # the logger: the keys, one line, the device totals
    from attend_infer_repeat_amd.evaluation import make_iw_logger
    got = make_iw_logger(air, lambda: (x, y), 2, 4, "test")(itr=3)
    assert set(got) == {"iw_bound", "elbo", "ess", "num_step_acc", "n_images"} and got["n_images"] == 2 * B
    assert all(math.isfinite(v) for v in got.values()) and 0.0 <= got["num_step_acc"] <= 1.0


def test_evaluate_iw_needs_the_engine(gpu_device):
    from attend_infer_repeat_amd import mnist_model
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    imgs, nums = synthetic_multi_mnist(4, (50, 50), 2, seed=0)
    air = mnist_model.AIRonMNIST(torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda(), max_steps=3)
    with pytest.raises(NotImplementedError, match="engine"):
        air.evaluate_iw(particles=2)


def test_training_script_iw_option(gpu_device, tmp_path, capsys):
    """--iw-particles 0 (the default) adds nothing to what the script prints and writes; K > 0 adds one line per log point and
    leaves the training run itself bit-identical."""
    import json
    import os
    import re
    from attend_infer_repeat_amd.scripts import multi_mnist
    common = ["--iters", "4", "--log-every", "2", "--save-every", "1000", "--synthetic-samples", "256", "--eval-batches", "1",
              "--summary-every", "0"]
    runs = {}
    for tag, extra in (("default", []), ("off", ["--iw-particles", "0"]), ("on", ["--iw-particles", "2"])):
        air = multi_mnist.main(common + ["--results-dir", str(tmp_path / tag)] + extra)
        air._engine.synchronize()
        printed = capsys.readouterr().out
        lines = [json.loads(l) for l in open(os.path.join(tmp_path, tag, "multi_mnist", "log.jsonl"))]
        runs[tag] = (air._engine.flat_params.clone(), printed, lines)
    strip = lambda s: re.sub(r"eval time = \S+s|\d+ images/s", "", s)
    assert strip(runs["off"][1]) == strip(runs["default"][1]) and "IW(" not in runs["off"][1]
    assert runs["off"][2] == runs["default"][2] and not any(l["data"].endswith("_iw") for l in runs["off"][2])
    iw = [l for l in runs["on"][2] if l["data"] == "test_iw"]
    assert [l["step"] for l in iw] == [0, 2, 4] and all(l["particles"] == 2 and l["n_images"] == 64 for l in iw)
    assert all(math.isfinite(l["iw_bound"]) and l["iw_bound"] >= l["elbo"] - 2e-5 * (abs(l["elbo"]) + 1) for l in iw)
    assert runs["on"][1].count("IW(2)") == 3
    assert torch.equal(runs["on"][0], runs["off"][0])


def test_bf16_log_weights_match_bf16_emulating_oracle(gpu_device):
    ocfg, B, K = O.AIRConfig(), 8, 8
    params, obs, noise = make_inputs(ocfg, B, K)
    with O.matmul_mode("bf16"):
        _, _, res = oracle_log_weights(ocfg, params, obs, noise, K, True)
        noise, moved = _separate_borderline_draws(noise, res)
        ref, n, res = oracle_log_weights(ocfg, params, obs, noise, K, True)
    ev = make_evaluator(ocfg, B, K, params, noise, mfma_dtype="bf16")
    out = ev.evaluate(obs.cuda(), sample_noise=False)
    ev.synchronize()
    assert ev.engine.cfg.mfma_dtype == "bf16"
    assert torch.equal(ev.engine.presence.cpu().double().reshape(-1), res["presence"].reshape(-1))
    assert torch.equal(out["num_steps"].cpu().reshape(-1).long(), n.long())
    err = rel_err(out["log_weights"].reshape(-1), ref)
    print("bf16 log w: worst / max = %.3e (%d borderline draws moved)" % (err, moved))
    assert err < 2e-3, err
