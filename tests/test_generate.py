"""GPU tests of scene generation (attend_infer_repeat_amd/generate.py, csrc/gen_kernels.hip): the ancestral draw of the latents
against float64, its count and latent statistics at 65 536 scenes, the decode chain against the float64 oracle and against the
engine's own canvas, the observation kernel against air_rng_fill's numbers, graph replay against eager, and the public surface
(AIRonMNIST.sample_scenes, make_prior_fig, scripts/multi_mnist.py --prior-samples, SceneSampler.dream).

Bars.  A latent is loc + scale * eps: two fp32 roundings (or one fused), each <= 2^-24 relative, so |got - ref| <= 1e-6 (|ref| + 1)
against float64 on the same fp32 inputs; the same bar holds for obs = mean + std * z.  The statistics use 5 standard errors of the
statistic itself (fixed seed: the outcome is deterministic).  The mean canvas is an output of the decoder + canvas kernels the
engine suite pins: that suite's per-sample output bars OUT_TOL = 1e-4 (worst element / tensor max) and OUT_L2 = 3e-5 (relative
L2); the bf16 case uses the bars of test_engine.py::test_bf16_path_at_batch_1024_matches_bf16_emulating_oracle."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

from fold_cases import philox_normals
from oracle import air_oracle as O
from test_engine import CONFIGS, OUT_L2, OUT_TOL, check_tensor, f64, l2_err, make_pair

pytestmark = pytest.mark.gpu

PRIORS = dict(what=(0.25, 1.5), scale=(0.625, 0.25), shift=(-0.125, 0.75))       # exactly representable in fp32
LATENT_SHAPES = [(3, 7, 50), (5, 6, 12), (1, 5, 5)]                           # the last: A % 4 != 0 -> the 4-byte vector path
F32_BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def engine_config(ocfg, mfma_dtype="f32", **kw):
    from attend_infer_repeat_amd.engine_config import EngineConfig
    fields = {f.name for f in dataclasses.fields(EngineConfig)}
    d = {k: v for k, v in dataclasses.asdict(ocfg).items() if k in fields}
    d.update(kw)
    return EngineConfig(mfma_dtype=mfma_dtype, **d)


def run_latents(table, u, eps_what, eps_where, n_in=None, guard=0.0, priors=PRIORS):
    """air_prior_latents alone on device tensors (current stream)"""
    from attend_infer_repeat_amd import _lib, hip as H
    T, R, A = eps_what.shape
    dev = eps_what.device
    out = dict(what=torch.full((T, R, A), float("nan"), device=dev), where=torch.full((T, R, 4), float("nan"), device=dev),
               presence=torch.full((T, R), float("nan"), device=dev), num_objects=torch.full((R,), -7, dtype=torch.int32, device=dev))
    st = H.lib().air_prior_latents(H._p(table), H._p(u), H._p(n_in), H._p(eps_what), H._p(eps_where), *priors["what"],
                                   *priors["scale"], *priors["shift"], float(guard), T, R, A, H._p(out["what"]), H._p(out["where"]),
                                   H._p(out["presence"]), H._p(out["num_objects"]), H._stream())
    _lib.check(st, "air_prior_latents")
    torch.cuda.synchronize()
    return out


def f64_counts(table, u):
    """n = #{c < T : cum_c <= (double)u * total}, running sums in index order"""
    w = [float(v) for v in table]
    T = len(w) - 1
    cum, acc = [], 0.0
    for v in w:
        acc += v
        cum.append(acc)
    return torch.tensor([sum(1 for c in range(T) if cum[c] <= float(np.float64(np.float32(x))) * cum[-1]) for x in u], dtype=torch.int64)


def f64_latents(eps_what, eps_where, priors=PRIORS):
    what = priors["what"][0] + priors["what"][1] * eps_what.double().cpu()
    loc = torch.tensor([priors["scale"][0], priors["shift"][0]] * 2, dtype=torch.float64)
    scale = torch.tensor([priors["scale"][1], priors["shift"][1]] * 2, dtype=torch.float64)
    return what, loc + scale * eps_where.double().cpu()


def check_latents(got, what_ref, where_ref):
    for k, ref in (("what", what_ref), ("where", where_ref)):
        err = ((got[k].double().cpu() - ref).abs() / (ref.abs() + 1.0)).max().item()
        print("%s: worst |got - ref| / (|ref| + 1) = %.3e" % (k, err))
        assert err <= 1e-6, (k, err)


def covering_uniforms(table, n_random, seed):
    """the midpoint of every CDF interval, u = 0, the largest float32 below 1, random draws"""
    w = np.asarray(table, np.float64)
    cum = np.cumsum(w) / w.sum()
    mids = [(a + b) / 2 for a, b, x in zip(np.concatenate([[0.0], cum[:-1]]), cum, w) if x > 0]
    rnd = np.random.default_rng(seed).random(n_random)
    return np.asarray(mids + [0.0, F32_BELOW_ONE] + list(rnd), np.float32)


# ---- 1. latents against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,R,A", LATENT_SHAPES)
def test_latents_match_f64(gpu_device, T, R, A):
    g = torch.Generator().manual_seed(100 * T + A)
    table = (torch.rand(T + 1, generator=g, dtype=torch.float64) + 0.1) * 3.0          # unnormalised
    n_u = -(-(T + 3 + 4) // R) * R                                # whole calls of R rows: every u of the cover + random fill
    us = covering_uniforms(table.tolist(), n_u - (T + 3), seed=T)
    seen = []
    for lo in range(0, n_u, R):
        u = torch.from_numpy(us[lo:lo + R].copy())
        eps_what, eps_where = torch.randn(T, R, A, generator=g), torch.randn(T, R, 4, generator=g)
        got = run_latents(table.cuda(), u.cuda(), eps_what.cuda(), eps_where.cuda())
        n = f64_counts(table.tolist(), u.tolist())
        assert torch.equal(got["num_objects"].cpu().long(), n), (u, got["num_objects"], n)
        assert torch.equal(got["presence"].cpu(), (torch.arange(T)[:, None] < n[None, :]).float())
        check_latents(got, *f64_latents(eps_what, eps_where))
        seen += n.tolist()
    assert sorted(set(seen)) == list(range(T + 1)), seen           # every count 0..T occurred
    assert f64_counts(table.tolist(), [0.0]).item() == 0 and f64_counts(table.tolist(), [F32_BELOW_ONE]).item() == T


def test_latents_zero_weights_given_counts_and_guard(gpu_device):
    T, R, A = 3, 7, 50
    g = torch.Generator().manual_seed(7)
    eps_what, eps_where = torch.randn(T, R, A, generator=g).cuda(), torch.randn(T, R, 4, generator=g)
    u = torch.tensor([0.0, F32_BELOW_ONE, 0.5, 0.25, 0.75, 1e-30, 0.999], dtype=torch.float32).cuda()
    t64 = lambda v: torch.tensor(v, dtype=torch.float64).cuda()
    # a weight of exactly zero is never drawn, also at u = 0
    got = run_latents(t64([0.0, 1.0, 0.0, 0.0]), u, eps_what, eps_where.cuda())
    assert got["num_objects"].tolist() == [1] * R and torch.equal(got["presence"].sum(0).cpu(), torch.ones(R))
    got = run_latents(t64([0.5, 0.5, 0.0, 0.0]), u, eps_what, eps_where.cuda())
    assert got["num_objects"].max().item() == 1 and got["num_objects"].tolist() == f64_counts([0.5, 0.5, 0.0, 0.0], u.tolist()).tolist()
    assert set(got["num_objects"].tolist()) == {0, 1}
    got = run_latents(t64([0.5, 0.0, 0.5, 0.0]), u, eps_what, eps_where.cuda())          # u = 0.5 sits ON a running sum: steps over the zero
    assert got["num_objects"].tolist() == f64_counts([0.5, 0.0, 0.5, 0.0], u.tolist()).tolist() and 1 not in got["num_objects"].tolist()
    # given counts: clipped to 0..T, neither the table nor u is read
    n_in = torch.tensor([0, 1, 2, 3, -2, 9, 3], dtype=torch.int32)
    got = run_latents(None, None, eps_what, eps_where.cuda(), n_in=n_in.cuda())
    assert torch.equal(got["num_objects"].cpu(), n_in.clamp(0, T))
    assert torch.equal(got["presence"].cpu(), (torch.arange(T)[:, None] < n_in.clamp(0, T)[None, :]).float())
    check_latents(got, *f64_latents(eps_what, eps_where))
    # guard_eps: |sx|, |sy| >= guard, sign kept, +guard for an exact zero; everything else unchanged
    loc, sc = PRIORS["scale"]
    eps_where[0, 0, 0] = -loc / sc                                 # sx = 0 exactly (0.625 - 0.25 * 2.5)
    eps_where[1, 2, 2] = (-0.03 - loc) / sc                        # sy = -0.03
    eps_where[2, 5, 0] = (0.05 - loc) / sc                         # sx = +0.05
    eps_where[0, 3, 1] = (0.01 - PRIORS["shift"][0]) / PRIORS["shift"][1]        # tx = 0.01: shifts are not guarded
    plain = run_latents(None, None, eps_what, eps_where.cuda(), n_in=n_in.cuda())
    guarded = run_latents(None, None, eps_what, eps_where.cuda(), n_in=n_in.cuda(), guard=0.1)
    pw, gw = plain["where"].cpu(), guarded["where"].cpu()
    assert pw[0, 0, 0].item() == 0.0 and (pw[..., 0::2].abs() < 0.1).sum().item() >= 3
    assert gw[..., 0::2].abs().min().item() >= 0.1
    assert gw[0, 0, 0].item() == pytest.approx(0.1) and gw[1, 2, 2].item() == pytest.approx(-0.1) and gw[2, 5, 0].item() == pytest.approx(0.1)
    small = torch.zeros_like(pw, dtype=torch.bool)
    small[..., 0::2] = pw[..., 0::2].abs() < 0.1
    assert torch.equal(gw[~small], pw[~small]) and abs(gw[0, 3, 1].item()) < 0.1
    assert torch.equal(guarded["what"], plain["what"]) and torch.equal(guarded["presence"], plain["presence"])


# ---- 2. count and latent statistics ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_noise():
    """Philox noise for 65 536 scenes of the tiny configuration (T = 3, A = 10), fixed seed"""
    from attend_infer_repeat_amd import hip as H
    T, R, A = 3, 65536, 10
    state = torch.tensor([1234, 0], dtype=torch.int64, device="cuda")
    normal = torch.zeros(T * R * 4 + T * R * A, device="cuda")
    u = torch.zeros(R, device="cuda")
    H.rng_fill(state, normal=normal, uniform=u, advance=False)
    torch.cuda.synchronize()
    return T, R, A, normal[:T * R * 4].view(T, R, 4), normal[T * R * 4:].view(T, R, A), u


@pytest.mark.parametrize("which", ["model_step_20000", "uniform"])
def test_count_frequencies_and_latent_moments(gpu_device, device_noise, which):
    from attend_infer_repeat_amd.engine_config import anneal_weight, geometric_prior_f64
    T, R, A, eps_where, eps_what, u = device_noise
    ocfg = CONFIGS["tiny"][0]
    assert (ocfg.max_steps, ocfg.n_appearance) == (T, A)
    if which == "uniform":
        table = [1.0] * (T + 1)
    else:
        s = anneal_weight(ocfg.nsp_init, ocfg.nsp_final, ocfg.nsp_anneal, 20000, ocfg.nsp_steps, ocfg.nsp_hold_init, ocfg.nsp_steps_div)
        table = geometric_prior_f64(s, T)
    got = run_latents(torch.tensor(table, dtype=torch.float64).cuda(), u, eps_what, eps_where)
    p = np.asarray(table) / np.sum(table)
    freq = torch.bincount(got["num_objects"].long(), minlength=T + 1).cpu().numpy() / R
    for c in range(T + 1):
        bound = 5 * math.sqrt(p[c] * (1 - p[c]) / R)
        print("n = %d: frequency %.6f, table %.6f, 5 se %.6f" % (c, freq[c], p[c], bound))
        assert abs(freq[c] - p[c]) <= bound, (c, freq[c], p[c])
    assert torch.equal(got["presence"].sum(0).long(), got["num_objects"].long())
    for name, x, (loc, scale) in (("what", got["what"], PRIORS["what"]), ("where scale", got["where"][..., 0::2], PRIORS["scale"]),
                                  ("where shift", got["where"][..., 1::2], PRIORS["shift"])):
        x = x.double().reshape(-1)
        N = x.numel()
        mean, var = x.mean().item(), x.var().item()
        print("%s: mean %.6f (prior %.6f, 5 se %.6f)  var %.6f (prior %.6f, 5 se %.6f)"
              % (name, mean, loc, 5 * scale / math.sqrt(N), var, scale ** 2, 5 * scale ** 2 * math.sqrt(2 / N)))
        assert abs(mean - loc) <= 5 * scale / math.sqrt(N), (name, mean)
        assert abs(var - scale ** 2) <= 5 * scale ** 2 * math.sqrt(2 / N), (name, var)


# ---- 3. decode against the float64 oracle ---------------------------------------------------------------------------------------
DECODE_CASES = {"tiny_r12": (CONFIGS["tiny"][0], 12), "rect_t5_r12": (CONFIGS["rect_t5"][0], 12), "mnist_r16": (O.AIRConfig(), 16)}


def prior_latents_host(ocfg, R, seed=31):
    """plain prior draws with n = r mod (T + 1): n = 0 and n = T are present"""
    T, A = ocfg.max_steps, ocfg.n_appearance
    g = torch.Generator().manual_seed(seed)
    what = ocfg.what_prior[0] + ocfg.what_prior[1] * torch.randn(T, R, A, generator=g)
    loc = torch.tensor([ocfg.where_scale_prior[0], ocfg.where_shift_prior[0]] * 2)
    scale = torch.tensor([ocfg.where_scale_prior[1], ocfg.where_shift_prior[1]] * 2)
    where = loc + scale * torch.randn(T, R, 4, generator=g)
    n = torch.arange(R) % (T + 1)
    presence = (torch.arange(T)[:, None] < n[None, :]).float()
    return what, where, presence, n


def oracle_mean(ocfg, params, what, where, presence):
    """mult * sum_t z_t * st_write(mlp(what_t), where_t) in float64"""
    T, R = presence.shape
    p = f64(params)
    layers = len(ocfg.glimpse_decoder_hidden) + 1
    canvas = torch.zeros(R, *ocfg.img_size, dtype=torch.float64)
    glimpses = []
    for t in range(T):
        dec = O.mlp(what[t].double(), p, "glimpse_decoder", layers, last_linear=True).reshape(R, *ocfg.crop_size)
        canvas = canvas + presence[t].double()[:, None, None] * O.st_write(dec, where[t].double(), ocfg.img_size)
        glimpses.append(dec)
    return ocfg.output_multiplier * canvas, torch.stack(glimpses)


def make_sampler(ocfg, R, params, mfma_dtype="f32", **kw):
    from attend_infer_repeat_amd.generate import SceneSampler
    s = SceneSampler(engine_config(ocfg, mfma_dtype), R, **kw)
    s.load_parameters(params)
    return s


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_decode_matches_f64_oracle(gpu_device, name):
    ocfg, R = DECODE_CASES[name]
    T = ocfg.max_steps
    params = O.init_params(ocfg, seed=1, bias_std=0.1)
    what, where, presence, n = prior_latents_host(ocfg, R)
    hand = T                                                       # row T has n = T: every step present
    assert n[hand] == T and n[0] == 0
    where[0, hand, 0] = 0.0                                        # sx = 0 on its first step: 1 / sx = inf, the step writes nothing
    s = make_sampler(ocfg, R, params)
    out = s.decode(what.cuda(), where.cuda(), presence.cuda())
    mean, glimpse = out["mean"].clone(), out["glimpse"].clone()
    ref, ref_glimpse = oracle_mean(ocfg, params, what, where, presence)
    assert torch.isfinite(ref).all() and torch.isfinite(mean).all()
    check_tensor("generate_decode", name, "out", "mean", mean, ref, OUT_TOL, OUT_L2)
    check_tensor("generate_decode", name, "out", "glimpse", glimpse, ref_glimpse, OUT_TOL, OUT_L2)
    for r in range(R):
        if n[r] == 0:
            assert mean[r].abs().max().item() == 0.0, r            # rows with n = 0 are exactly zero
    assert ref.abs().max().item() > 0.0
    without = presence.clone()
    without[0, hand] = 0.0                                         # the hand-made row: the same canvas as without that step
    again = s.decode(what.cuda(), where.cuda(), without.cuda())["mean"]
    assert torch.equal(again[hand], mean[hand])


def test_decode_bf16_matches_bf16_emulating_oracle(gpu_device):
    ocfg, R = DECODE_CASES["mnist_r16"]
    params = O.init_params(ocfg, seed=1, bias_std=0.1)
    what, where, presence, _ = prior_latents_host(ocfg, R)
    s = make_sampler(ocfg, R, params, mfma_dtype="bf16")
    assert s.cfg.mfma_dtype == "bf16" and all(e[2] == "air_gemm_bf16" for e in s._plans["decode"][:3])
    mean = s.decode(what.cuda(), where.cuda(), presence.cuda())["mean"].cpu().double().reshape(-1)
    with O.matmul_mode("bf16"):
        ref, _ = oracle_mean(ocfg, params, what, where, presence)
    ref = ref.reshape(-1)
    err = (mean - ref).abs() / (ref.abs().max() + 1e-12)
    p999 = torch.quantile(err, 0.999).item()
    print("bf16 mean: l2 %.3e p999 %.3e max %.3e" % (l2_err(mean, ref), p999, err.max().item()))
    assert l2_err(mean, ref) < 2e-3 and p999 < 2e-3 and err.max().item() < 0.1


# ---- 4. decode of the engine's own latents --------------------------------------------------------------------------------------
def test_decode_of_engine_latents_gives_the_engine_canvas(gpu_device):
    from attend_infer_repeat_amd.generate import SceneSampler
    ocfg, B = CONFIGS["mnist_b8"]
    eng, params, obs, noise = make_pair(ocfg, B)
    eng.forward(sample_noise=False)
    ref = eng.outputs()["final_canvas"].clone()
    assert eng.presence.sum().item() > 0
    s = SceneSampler(eng.cfg, B, seed=5)
    s.load_from(eng)
    mean = s.decode(eng.what, eng.where, eng.presence)["mean"]
    s.synchronize()
    assert s.global_step == eng.global_step == 20000 and int(s.step_dev.item()) == 20000
    assert torch.equal(s.params["glimpse_decoder/1/w"], eng.params["glimpse_decoder/1/w"])
    check_tensor("generate_engine_latents", "mnist_b8", "out", "mean", mean, ref.double().cpu(), OUT_TOL, OUT_L2)
    with pytest.raises(ValueError, match="architecture"):
        SceneSampler(engine_config(CONFIGS["rect_t5"][0]), B).load_from(eng)


# ---- 5. air_observe ------------------------------------------------------------------------------------------------------------
def run_observe(canvas, mult, std, state, counter_base, clamp=(float("nan"), float("nan")), want_mean=True, want_obs=True):
    from attend_infer_repeat_amd import _lib, hip as H
    n = canvas.numel()
    mean = torch.full((n,), float("nan"), device=canvas.device) if want_mean else None
    obs = torch.full((n,), float("nan"), device=canvas.device) if want_obs else None
    st = H.lib().air_observe(H._p(canvas), float(mult), float(std), H._p(state), int(counter_base), float(clamp[0]), float(clamp[1]),
                             H._p(mean), H._p(obs), n, H._stream())
    _lib.check(st, "air_observe")
    torch.cuda.synchronize()
    return mean, obs


@pytest.mark.parametrize("n", [4 * 625, 4 * 625 + 3, 4 * (2048 * 256 + 1000) + 1])    # aligned body; + tail; more quads than grid threads
def test_observe_matches_rng_fill_numbers(gpu_device, n):
    mult, std, seed, offset, base = 0.5, 0.3, 99, 1000, 77
    canvas = torch.rand(n, generator=torch.Generator().manual_seed(n % 1000)).cuda() * 2.4 - 0.2
    state = torch.tensor([seed, offset], dtype=torch.int64, device="cuda")
    # std = 0: no draw; obs == mean == torch's mult * canvas, bit for bit
    mean, obs = run_observe(canvas, mult, 0.0, None, base)
    assert torch.equal(mean, mult * canvas) and torch.equal(obs, mean)
    # std = 0.3: element i gets element i of air_rng_fill at {seed, offset + counter_base}
    z = philox_normals(seed, offset + base, n)
    mean, obs = run_observe(canvas, mult, std, state, base)
    ref = mult * canvas.double() + float(np.float32(std)) * z.double()
    err = ((obs.double() - ref).abs() / (ref.abs() + 1.0)).max().item()
    print("n = %d: worst |obs - ref| / (|ref| + 1) = %.3e, noise std %.4f" % (n, err, ((obs - mean) / std).std().item()))
    assert err <= 1e-6 and torch.equal(mean, mult * canvas)
    assert state.tolist() == [seed, offset]                        # the entry does not advance the state
    # clamp to [0, 1] holds and leaves interior values unchanged
    _, clamped = run_observe(canvas, mult, std, state, base, clamp=(0.0, 1.0))
    assert clamped.min().item() >= 0.0 and clamped.max().item() <= 1.0
    inside = (obs > 0.0) & (obs < 1.0)
    assert 0 < inside.sum().item() < n and torch.equal(clamped[inside], obs[inside])
    assert torch.equal(clamped[~inside], obs[~inside].clamp(0.0, 1.0))
    _, lower = run_observe(canvas, mult, std, state, base, clamp=(0.0, float("nan")))    # one NaN bound: that side is open
    assert torch.equal(lower, obs.clamp(min=0.0))
    # either output alone
    only_mean, none = run_observe(canvas, mult, std, state, base, want_obs=False)
    assert none is None and torch.equal(only_mean, mean)
    none, only_obs = run_observe(canvas, mult, std, state, base, want_mean=False)
    assert none is None and torch.equal(only_obs, obs)
    if n < 10000:
        # buffers that are only 4-byte aligned take the scalar form: the same numbers (z_i counts from the pointer given)
        shifted = torch.zeros(n + 1, device="cuda")
        shifted[1:] = canvas
        m2, o2 = run_observe(shifted[1:], mult, std, state, base)
        assert torch.equal(m2, mean) and torch.equal(o2, obs)


# ---- 6. the sampler as a graph --------------------------------------------------------------------------------------------------
KEYS = ("obs", "mean", "what", "where", "presence", "num_objects", "glimpse")


def test_sampler_graph_replay_equals_eager_and_philox_bookkeeping(gpu_device):
    ocfg, R = CONFIGS["rect_t5"][0], 12
    T, A = ocfg.max_steps, ocfg.n_appearance
    params = O.init_params(ocfg, seed=1, bias_std=0.1)
    eager = make_sampler(ocfg, R, params, seed=3, count_probs="uniform")
    graph = make_sampler(ocfg, R, params, seed=3, count_probs="uniform")
    graph.capture()
    assert set(graph._graphs) == set(graph._plans)
    state0 = graph.rng_state.clone()
    kept = []
    for _ in range(2):
        a, b = eager.sample(), graph.sample()
        eager.synchronize(); graph.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k                     # same seed, same state: identical bits, replay == eager
        kept.append({k: b[k].clone() for k in KEYS})
    for k in ("obs", "mean", "what", "where"):
        assert not torch.equal(kept[0][k], kept[1][k]), k          # fresh noise per call
    assert graph.rng_state.tolist() == [3, 2 * (graph.q_lat + graph.q_pix)]
    assert graph.q_lat == (T * R * (4 + A) + 3) // 4 + (R + 3) // 4 and graph.q_pix == (R * ocfg.n_pix + 3) // 4
    # the pixel noise of the first call: element i of air_rng_fill at {seed, q_lat}
    z = philox_normals(3, graph.q_lat, R * ocfg.n_pix).reshape(kept[0]["mean"].shape)
    ref = kept[0]["mean"].double() + float(np.float32(ocfg.output_std)) * z.double()
    assert ((kept[0]["obs"].double() - ref).abs() / (ref.abs() + 1.0)).max().item() <= 1e-6
    # restoring the state reproduces the first call
    graph._copy_in(graph.rng_state, state0)
    again = graph.sample()
    for k in KEYS:
        assert torch.equal(again[k], kept[0][k]), k
    # given counts: a scalar, and one per scene (clipped)
    assert graph.sample(num_objects=2)["num_objects"].tolist() == [2] * R
    counts = torch.arange(R, dtype=torch.int64) - 2
    out = graph.sample(num_objects=counts)
    assert torch.equal(out["num_objects"].cpu().long(), counts.clamp(0, T))
    assert torch.equal(out["presence"].sum(0).cpu().long(), counts.clamp(0, T))
    # the plan is what launch_count says
    lc = graph.launch_count()
    assert lc == {"rng_fill": 1, "prior_latents": 1, "decoder": len(ocfg.glimpse_decoder_hidden) + 1, "canvas": 1, "observe": 1,
                  "rng_advance": 1}
    names = [e[2] for e in graph._plans[(True, False)]]
    assert names == (["air_rng_fill", "air_prior_latents"] + ["air_linear_fwd"] * lc["decoder"]
                     + ["air_canvas_unroll_fwd", "air_observe", "air_rng_advance"]) and sum(lc.values()) == len(names)
    assert sum(graph.launch_count(sample_noise=False).values()) == len(graph._plans[(False, False)]) == len(names) - 1
    graph.release_graphs()
    assert graph._graphs == {}


def test_sampler_with_injected_noise_reproduces_latents_and_decode_end_to_end(gpu_device):
    ocfg, R = CONFIGS["tiny"][0], 12
    T, A = ocfg.max_steps, ocfg.n_appearance
    params = O.init_params(ocfg, seed=1, bias_std=0.1)
    table = [0.1, 0.4, 0.2, 0.3]
    s = make_sampler(ocfg, R, params, count_probs=table, pixel_noise=False)
    s.capture()
    g = torch.Generator().manual_seed(17)
    eps_what, eps_where = torch.randn(T, R, A, generator=g), torch.randn(T, R, 4, generator=g)
    u = torch.from_numpy(covering_uniforms(table, R - (T + 3), seed=3))
    s.set_noise(eps_what.cuda(), eps_where.cuda(), u.cuda())
    out = {k: v.clone() for k, v in s.sample(sample_noise=False).items()}
    n = f64_counts(table, u.tolist())
    assert sorted(set(n.tolist())) == [0, 1, 2, 3]
    assert torch.equal(out["num_objects"].cpu().long(), n)
    assert torch.equal(out["presence"].cpu(), (torch.arange(T)[:, None] < n[None, :]).float())
    pri = dict(what=ocfg.what_prior, scale=ocfg.where_scale_prior, shift=ocfg.where_shift_prior)
    check_latents(out, *f64_latents(eps_what, eps_where, pri))
    ref, _ = oracle_mean(ocfg, params, out["what"].cpu(), out["where"].cpu(), out["presence"].cpu())
    check_tensor("generate_end_to_end", "tiny_r12", "out", "mean", out["mean"], ref, OUT_TOL, OUT_L2)
    assert torch.equal(out["obs"], out["mean"])                   # pixel_noise=False
    assert s.rng_state.tolist() == [0, s.q_lat] and s.q_pix == 0


def test_model_count_table_is_the_engines(gpu_device):
    """count_probs=None: air_steps_prior at the sampler's step -- the table the engine's forward leaves in prior_dev"""
    ocfg, B = CONFIGS["tiny"]
    eng, params, obs, noise = make_pair(ocfg, B)
    eng.forward(sample_noise=False)
    eng.synchronize()
    s = make_sampler(ocfg, 4, params)
    s.set_global_step(20000)
    s.synchronize()
    assert torch.equal(s.table, eng.prior_dev) and "20000" in s.count_label
    s.set_count_probs("uniform"); s.synchronize()
    assert s.table.tolist() == [1.0] * 4 and s.count_label == "uniform"
    s.set_count_probs(None); s.synchronize()
    assert torch.equal(s.table, eng.prior_dev)


# ---- 7. through the public surface ----------------------------------------------------------------------------------------------
def _mnist_air(B=8):
    from attend_infer_repeat_amd import mnist_model, utils
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    AD = utils.AttrDict
    imgs, nums = synthetic_multi_mnist(B, (50, 50), 2, seed=0)
    x, y = torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda()
    torch.manual_seed(0)
    air = mnist_model.AIRonMNIST(x, y, max_steps=3, explore_eps=1e-3, steps_pred_hidden=[128, 64], transform_var_bias=.5,
                                 step_bias=.75, output_multiplier=.5)
    nsp = AD(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    ts, _ = air.train_step(1e-4, 0., AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp)
    return air, ts


def test_sample_scenes_and_prior_figure_on_the_model(gpu_device):
    from matplotlib.patches import Rectangle
    from attend_infer_repeat_amd.evaluation import attention_box, make_prior_fig
    air, ts = _mnist_air(8)
    ts()
    before = air._engine.flat_params.clone()
    assert air.sample_scenes(6, count_probs="uniform") is air
    T, N = 3, 6
    shapes = dict(generated_obs=(N, 50, 50), generated_mean=(N, 50, 50), generated_num_objects=(N,), generated_what=(T, N, 50),
                  generated_where=(T, N, 4), generated_presence=(T, N))
    for k, shape in shapes.items():
        assert tuple(getattr(air, k).shape) == shape, k
    assert torch.equal(air.generated_presence.sum(0).long(), air.generated_num_objects.long())
    assert torch.isfinite(air.generated_obs).all() and not torch.equal(air.generated_obs, air.generated_mean)
    s = air.scene_sampler()
    assert s.R == 6 and air.scene_sampler(6) is s and s._graphs
    assert torch.equal(s.params["glimpse_decoder/0/w"], air._engine.params["glimpse_decoder/0/w"]) and int(s.step_dev.item()) == 1
    assert air.sample_scenes(num_objects=2).generated_num_objects.tolist() == [2] * N
    assert torch.equal(air._engine.flat_params, before)           # the training engine is only read
    # the figure: row 0 the mean canvases with one box per present step, rows 1..T the decoded glimpses; caption = the count table
    fig = make_prior_fig(air, n_samples=4, count_probs="uniform")
    host = lambda t: t.detach().cpu().numpy()
    mean, glimpse, pres, where = (host(getattr(air, "generated_" + k)) for k in ("mean", "glimpse", "presence", "where"))
    axes = np.array(fig.axes).reshape(T + 1, 4)
    n_boxes = 0
    for col in range(4):
        ax = axes[0, col]
        assert np.array_equal(ax.images[0].get_array(), mean[col]) and ax.images[0].get_clim() == (0, 1)
        boxes = [p for p in ax.patches if isinstance(p, Rectangle)]
        present = [t for t in range(T) if pres[t, col] > .5]
        assert len(boxes) == len(present)
        for r, t in zip(boxes, present):
            left, top, bw, bh = attention_box(where[t, col], 50, 50)
            assert np.allclose([r.get_x(), r.get_y(), r.get_width(), r.get_height()], [left - .5, top - .5, bw, bh], atol=1e-4)
            n_boxes += 1
        for t in range(T):
            assert np.array_equal(axes[1 + t, col].images[0].get_array(), glimpse[t, col])
            assert axes[1 + t, col].get_title() == str(int(pres[t, col]))
    assert n_boxes == int(pres[:, :4].sum())
    assert "uniform" in fig._suptitle.get_text()
    assert air.scene_sampler(5).R == 5                              # another size: rebuilt


def test_sample_scenes_needs_the_engine(gpu_device):
    from attend_infer_repeat_amd import mnist_model
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    imgs, nums = synthetic_multi_mnist(4, (50, 50), 2, seed=0)
    air = mnist_model.AIRonMNIST(torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda(), max_steps=3)
    with pytest.raises(NotImplementedError, match="engine"):
        air.sample_scenes(4)


def test_training_script_prior_samples_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    multi_mnist.main(["--iters", "2", "--log-every", "2", "--save-every", "1000", "--synthetic-samples", "256", "--eval-batches", "1",
                      "--summary-every", "0", "--prior-samples", "4", "--figures", "--results-dir", str(tmp_path)])
    logdir = os.path.join(tmp_path, "multi_mnist")
    lines = [json.loads(l) for l in open(os.path.join(logdir, "log.jsonl"))]
    prior = [l for l in lines if l["data"] == "prior_samples"]
    assert [l["step"] for l in prior] == [0, 2]
    for l in prior:
        assert l["n_scenes"] == 4 and len(l["count_hist"]) == 4 and sum(l["count_hist"]) == 4 and l["count_probs"] == "model"
    for step in (0, 2):
        assert os.path.getsize(os.path.join(logdir, "prior_fig_%d.png" % step)) > 10_000
    assert capsys.readouterr().out.count("prior samples") == 2


def test_dream_fills_a_dataset_the_engine_trains_on(gpu_device):
    from attend_infer_repeat_amd.engine import AIREngine, EngineConfig
    from attend_infer_repeat_amd.generate import SceneSampler
    cfg = EngineConfig()
    eng = AIREngine(cfg, 8, seed=2)
    s = SceneSampler(cfg, 8, seed=4, count_probs="uniform", clamp=(0.0, 1.0))
    s.load_from(eng)
    s.capture()
    data, nums = s.dream(20)
    torch.cuda.synchronize()
    assert tuple(data.shape) == (20, 50, 50) and tuple(nums.shape) == (20,) and data.dtype == torch.float32
    assert 0 <= nums.min().item() and nums.max().item() <= cfg.max_steps and len(set(nums.tolist())) > 1
    assert torch.isfinite(data).all() and data.min().item() >= 0.0 and data.max().item() <= 1.0
    assert not torch.equal(data[:8], data[8:16])                    # chunks are fresh draws
    assert s.rng_state.tolist() == [4, 3 * (s.q_lat + s.q_pix)]
    eng.attach_dataset(data)
    eng.train_step()
    loss = eng.outputs()["loss"]
    assert torch.isfinite(loss).all(), loss
