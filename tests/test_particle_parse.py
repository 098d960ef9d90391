"""GPU tests of best-of-K scene parsing (attend_infer_repeat_amd/particle_parse.py, csrc/particle_kernels.hip): the selection rule
and the gather on crafted scores against a numpy float64 restatement, log q(z | x) against the float64 oracle, the spread of `where`
against numpy float64 on the kernel's own inputs, ParticleParser end to end against the oracle under three noise settings, K = 1 at
the mode against SceneParser, graph replay against eager, and the public surface.

Bars.  log q is a sum of the same per-sample outputs as log w (test_iw_eval.py): that suite's OUT_TOL = 1e-4 (worst element / tensor
max) and OUT_L2 = 3e-5 (relative L2); bf16: the 2e-3 of test_bf16_log_weights_match_bf16_emulating_oracle.  A score is log w or
log w + log q, each held to OUT_TOL, so the device can confuse two particles only when the oracle's scores lie within
m = 2 OUT_TOL max|oracle score| of each other: the device's winner must be within m of the oracle's best, and equal to it where the
oracle's top-two gap exceeds 2 m.  The spread kernel sees the SAME fp32 inputs as its float64 reference and works in float64 itself
(only the summation order and the closing rounding to fp32 differ): 1e-6 (|ref| + 1), the bar test_parse.py uses for a float64
quantity rounded to fp32; NaN exactly where the reference has NaN."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import air_oracle as O
from test_engine import OUT_L2, OUT_TOL, _separate_borderline_draws, check_tensor, rel_err
from test_iw_eval import CASES, GSTEP, engine_config, f64_reduce, make_inputs, oracle_log_weights
from test_parse import MASK_THRESHOLD, SENTINEL_F, SENTINEL_I, _mnist_air, _train_state, e2e_case, make_parser, mode_noise, \
    run_objects, run_render

pytestmark = pytest.mark.gpu

CRITERIA = {"weight": 0, "joint": 1}


def same_bits(a, b):
    """torch.equal that lets NaN equal NaN (where_mean / where_std of a step no particle has)"""
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0),
                                                                                                  torch.nan_to_num(b, nan=0.0))
    return torch.equal(a, b)


# ---- 1. selection and gather on crafted scores ----------------------------------------------------------------------------------
def f64_select(lw, lq, criterion):
    """the rule restated in numpy float64: (k*, degenerate, (float32) score at k* or NaN)"""
    s = lw.astype(np.float64) + (lq.astype(np.float64) if criterion == "joint" else 0.0)
    B = s.shape[0]
    best, deg, score = np.zeros(B, np.int64), np.zeros(B, np.int64), np.full(B, np.nan, np.float32)
    for b in range(B):
        valid = ~np.isnan(s[b])
        if not valid.any():
            deg[b] = 1
            continue
        m = s[b][valid].max()
        best[b] = int(np.nonzero(valid & (s[b] == m))[0][0])
        with np.errstate(over="ignore"):
            score[b] = np.float32(s[b, best[b]])
    return best, deg, score


N_PATTERNS = 7


def crafted_scores(B, K, seed):
    """[B, K] fp32 log_w, log_q: the first rows walk through the seven crafted patterns (twice when B allows, B = 1 gets the last
    one), the rest is random with repeated values (coarse grid: exact ties occur)"""
    rng = np.random.default_rng(seed)
    lw = (np.round(rng.normal(size=(B, K)) * 4) / 2 - 50).astype(np.float32)
    lq = (np.round(rng.normal(size=(B, K)) * 4) / 2 - 20).astype(np.float32)
    shift = N_PATTERNS - 1 if B == 1 else 0
    last, mid = K - 1, K // 2
    for b in range(min(B, 2 * N_PATTERNS)):
        p = (b + shift) % N_PATTERNS
        if p == 0:                                                 # all scores equal
            lw[b], lq[b] = -37.25, -3.5
        elif p == 1:                                               # an exact tie of the first and the last k above the rest
            lw[b, 0], lq[b, 0] = 10.0, 1.0
            lw[b, last], lq[b, last] = 10.0, 1.0
        elif p == 2:                                               # one NaN where the maximum would be
            lw[b, mid] = np.nan
            lq[b, mid] = 1000.0
        elif p == 3:                                               # all NaN
            lw[b] = np.nan
        elif p == 4:                                               # -inf everywhere: an ordinary value, k* = 0, not degenerate
            lw[b] = -np.inf
        elif p == 5:                                               # +inf at the middle and the last k; -inf at the first
            lw[b, 0] = -np.inf
            lw[b, mid] = lw[b, last] = np.inf
        else:                                                      # fp32 would round both sums to 1e4: float64 separates them
            lw[b, 0], lq[b, 0] = 1e4, 1e-4
            lw[b, last], lq[b, last] = 1e4, 1.5e-4
    return lw, lq


def run_select(lw, lq, n, where, what, prob, glimpse, criterion):
    """air_particle_select alone on device tensors (current stream); every output starts as a sentinel fill"""
    from attend_infer_repeat_amd import _lib, hip as Hh
    B, K = lw.shape
    T, R, A = what.shape
    G = glimpse.shape[-1]
    dev = what.device
    ff = lambda *s: torch.full(s, SENTINEL_F, device=dev)
    fi = lambda *s: torch.full(s, SENTINEL_I, dtype=torch.int32, device=dev)
    out = dict(best_particle=fi(B), best_score=ff(B), num_objects_in=fi(B), degenerate=fi(B), where=ff(T, B, 4), what=ff(T, B, A),
               presence_prob=ff(T, B), glimpse=ff(T, B, G))
    p = Hh._p
    st = Hh.lib().air_particle_select(p(lw), p(lq), p(n), p(where), p(what), p(prob), p(glimpse), T, R, K, A, G, CRITERIA[criterion],
                                      p(out["best_particle"]), p(out["best_score"]), p(out["num_objects_in"]), p(out["degenerate"]),
                                      p(out["where"]), p(out["what"]), p(out["presence_prob"]), p(out["glimpse"]), Hh._stream())
    _lib.check(st, "air_particle_select")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("A,G", [(5, 6), (5, 400), (12, 6), (12, 400)])      # A, h*w: the 4-byte and the 16-byte gather of each
@pytest.mark.parametrize("K", [1, 5, 64, 65, 200])                          # 65, 200: past the 64-lane stride
@pytest.mark.parametrize("B", [1, 7, 300])
def test_selection_and_gather_on_crafted_scores(gpu_device, B, K, A, G):
    T, R = 3, B * K
    lw_h, lq_h = crafted_scores(B, K, seed=1000 * B + K)
    g = torch.Generator(device="cuda").manual_seed(B + K + A + G)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    where, what, prob, glimpse = rnd(T, R, 4), rnd(T, R, A), rnd(T, R), rnd(T, R, G)
    n = torch.randint(0, T + 1, (B, K), generator=g, device="cuda").int()
    lw, lq = torch.from_numpy(lw_h).cuda(), torch.from_numpy(lq_h).cuda()
    ar = torch.arange(B, device="cuda")
    for criterion in ("joint", "weight"):
        got = run_select(lw, lq if criterion == "joint" else None, n, where, what, prob, glimpse, criterion)
        best, deg, score = f64_select(lw_h, lq_h, criterion)
        assert np.array_equal(got["best_particle"].cpu().numpy(), best), criterion
        assert np.array_equal(got["degenerate"].cpu().numpy(), deg), criterion
        assert np.array_equal(got["best_score"].cpu().numpy(), score, equal_nan=True), criterion
        ks = torch.from_numpy(best).cuda()
        assert torch.equal(got["num_objects_in"], n[ar, ks])
        pick = lambda x: x.reshape(T, B, K, -1)[:, ar, ks]
        assert torch.equal(got["where"], pick(where)) and torch.equal(got["what"], pick(what))
        assert torch.equal(got["presence_prob"], pick(prob)[..., 0]) and torch.equal(got["glimpse"], pick(glimpse))
    if B >= N_PATTERNS and K >= 2:                                 # the crafted rows are what they claim to be
        bj, dj, _ = f64_select(lw_h, lq_h, "joint")
        bw, dw, _ = f64_select(lw_h, lq_h, "weight")
        assert bj[0] == 0 and bj[1] == 0 and dj[3] == 1 and dw[3] == 1 and bj[4] == 0 and dj[4] == 0 and bj[5] == K // 2
        assert bj[2] != K // 2 and dj[2] == 0
        assert bj[6] == K - 1 and bw[6] == 0                        # float64 separates what fp32 (1e4 + 1e-4 == 1e4) cannot
        assert np.float32(1e4) + np.float32(1.5e-4) == np.float32(1e4)


# ---- shared: the oracle on the K-tiled images --------------------------------------------------------------------------------
SETTINGS = ("a", "b", "c")
_ORACLE = {}


def setting_noise(noise, setting):
    """(a) the oracle's noise as drawn; (b) every presence draw succeeds: n = T everywhere; (c) every draw fails: n = 0 everywhere"""
    if setting == "a":
        return noise
    return dict(noise, u_pres=torch.full_like(noise["u_pres"], -1.0 if setting == "b" else 2.0))


def oracle_log_q(ocfg, res, n):
    """log q(z | x) [R] in float64 from the oracle's outputs"""
    N = torch.distributions.Normal
    T = ocfg.max_steps
    R = n.shape[0]
    z = res["presence"].reshape(T, R)
    lq_what = N(res["what_loc"], res["what_scale"]).log_prob(res["what"]).sum(-1).reshape(T, R)
    lq_where = N(res["where_loc"], res["where_scale"]).log_prob(res["where"]).sum(-1).reshape(T, R)
    log_qn = O.num_steps_log_prob(res["num_steps_posterior"].double(), n)
    return log_qn + (z * (lq_what + lq_where)).sum(0)


def oracle_case(name, setting, mode="f32"):
    """(ocfg, B, K, params, obs, noise, log w [B, K], log q [B, K], n [B, K], res), computed once per case and shared (read-only)"""
    key = (name, setting, mode)
    if key not in _ORACLE:
        ocfg, B, K = CASES[name]
        params, obs, noise = make_inputs(ocfg, B, K)
        noise = setting_noise(noise, setting)
        logw, n, res = oracle_log_weights(ocfg, params, obs, noise, K, True)
        logq = oracle_log_q(ocfg, res, n)
        _ORACLE[key] = (ocfg, B, K, params, obs, noise, logw.reshape(B, K), logq.reshape(B, K), n.reshape(B, K).long(), res)
    return _ORACLE[key]


def make_particle_parser(ocfg, B, K, params, noise=None, select="joint", mfma_dtype="f32", seed=0, **kw):
    from attend_infer_repeat_amd.particle_parse import ParticleParser
    ps = ParticleParser(engine_config(ocfg, mfma_dtype), B, K, select=select, seed=seed, mask_threshold=MASK_THRESHOLD, **kw)
    ps.load_parameters(params)
    if noise is not None:
        ps.engine.set_noise(noise["eps_where"].cuda(), noise["eps_what"].cuda(), noise["u_pres"].cuda())
    ps.set_global_step(GSTEP)
    return ps


# ---- 2. log q against the float64 oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_b6_k5", "mnist_b8_k8", "rect_t5_b3_k4"])
def test_log_q_matches_f64_oracle(gpu_device, name):
    ocfg, B, K, params, obs, noise, logw, logq, n, res = oracle_case(name, "a")
    ps = make_particle_parser(ocfg, B, K, params, noise)
    out = ps.parse(obs.cuda(), sample_noise=False)
    ps.synchronize()
    T = ocfg.max_steps
    assert torch.equal(ps.engine.presence.cpu().double().reshape(T, B * K), res["presence"].reshape(T, B * K))
    assert torch.equal(out["num_steps"].cpu().long(), n)
    counts = torch.bincount(n.reshape(-1), minlength=T + 1)
    print("particles per n:", counts.tolist(), "log q range %.1f .. %.1f" % (logq.min().item(), logq.max().item()))
    assert counts[0] > 0 and counts[T] > 0 and counts[1:T].sum() > 0, counts       # a mask error cannot hide
    assert torch.isfinite(logq).all()
    got = out["log_q"].reshape(-1)
    print("log q: max %.3e l2 %.3e" % (rel_err(got, logq), ((got.cpu().double() - logq.reshape(-1)).norm() / logq.norm()).item()))
    check_tensor("particle_parse", name, "out", "log_q", got, logq.reshape(-1), OUT_TOL, OUT_L2)
    check_tensor("particle_parse", name, "out", "log_weights", out["log_weights"].reshape(-1), logw.reshape(-1), OUT_TOL, OUT_L2)


# ---- 3. the spread against numpy float64 on the kernel's own inputs --------------------------------------------------------------
def f64_spread(lw, n, where):
    """lw [B, K] fp32, n [B, K] int, where [T, B*K, 4] fp32 -> where_mean, where_std [T, B, 4], presence_iw [T, B] in numpy float64"""
    lw, n = lw.detach().cpu().numpy().astype(np.float64), n.detach().cpu().numpy()
    B, K = lw.shape
    x = where.detach().cpu().numpy().astype(np.float64)
    T = x.shape[0]
    x = x.reshape(T, B, K, 4)
    w = np.exp(lw - lw.max(1, keepdims=True))
    total = w.sum(1)
    mean, std, share = np.zeros((T, B, 4)), np.zeros((T, B, 4)), np.zeros((T, B))
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            wt = w * (n > t)
            W = wt.sum(1)
            mean[t] = (wt[:, :, None] * x[t]).sum(1) / W[:, None]
            var = (wt[:, :, None] * (x[t] - mean[t][:, None, :]) ** 2).sum(1) / W[:, None]
            std[t] = np.sqrt(np.where(var < 0, 0.0, var))
            share[t] = W / total
    return dict(where_mean=mean, where_std=std, presence_iw=share)


def check_spread(got, ref):
    for k, r in ref.items():
        g = got[k].detach().cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(r)), k
        fin = ~np.isnan(r)
        err = (np.abs(g[fin] - r[fin]) / (np.abs(r[fin]) + 1.0)).max() if fin.any() else 0.0
        print("spread %s: worst |got - ref| / (|ref| + 1) = %.3e, %d NaN" % (k, err, int((~fin).sum())))
        assert err <= 1e-6, (k, err)
    assert (got["where_std"][~torch.isnan(got["where_std"])] >= 0).all()


def run_spread(lw, n, where):
    """air_particle_spread alone on device tensors (current stream)"""
    from attend_infer_repeat_amd import _lib, hip as Hh
    B, K = lw.shape
    T = where.shape[0]
    dev = lw.device
    out = dict(where_mean=torch.full((T, B, 4), SENTINEL_F, device=dev), where_std=torch.full((T, B, 4), SENTINEL_F, device=dev),
               presence_iw=torch.full((T, B), SENTINEL_F, device=dev))
    p = Hh._p
    st = Hh.lib().air_particle_spread(p(lw), p(n), p(where), T, B * K, K, p(out["where_mean"]), p(out["where_std"]),
                                      p(out["presence_iw"]), Hh._stream())
    _lib.check(st, "air_particle_spread")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["mnist_b8_k8", "tiny_b6_k5"])
def test_spread_matches_f64_on_the_kernels_inputs(gpu_device, name):
    ocfg, B, K, params, obs, noise, *_ = oracle_case(name, "a")
    ps = make_particle_parser(ocfg, B, K, params, noise)
    out = ps.parse(obs.cuda(), sample_noise=False)
    ps.synchronize()
    check_spread(out, f64_spread(out["log_weights"], out["num_steps"], ps.engine.where))
    again = run_spread(out["log_weights"], out["num_steps"], ps.engine.where)      # the entry on its own gives the same bits
    for k in again:
        assert same_bits(again[k], out[k]), k
    # the weight share of the particles that have step t is the importance-weighted P(n > t)
    tail = torch.flip(torch.cumsum(torch.flip(out["num_steps_posterior_iw"].double(), (1,)), 1), (1,))[:, 1:]      # [B, T]
    assert (out["presence_iw"].double().t() - tail).abs().max() <= 2e-5


def test_spread_on_crafted_blocks(gpu_device):
    T = 3
    g = torch.Generator().manual_seed(7)
    for B, K in ((5, 7), (3, 65), (2, 200), (4, 1)):
        where = torch.randn(T, B * K, 4, generator=g).cuda()
        # a step nobody has: n <= 1 everywhere, so S_1 and S_2 are empty -> NaN mean and std, share 0; image 0 has no object at all
        lw = (torch.randn(B, K, generator=g) * 3 - 40).cuda()
        n = torch.randint(0, 2, (B, K), generator=g).int()
        n[0] = 0
        n[-1, 0] = 1
        got = run_spread(lw, n.cuda(), where)
        check_spread(got, f64_spread(lw, n, where))
        assert torch.isnan(got["where_mean"][1:]).all() and torch.isnan(got["where_std"][1:]).all()
        assert (got["presence_iw"][1:] == 0).all() and torch.isnan(got["where_mean"][0, 0]).all()
        assert not torch.isnan(got["where_mean"][0, -1]).any()
        # all the weight on one particle (the others 1000 nats below: exp underflows to 0 in float64): mean = its row, std = 0
        lw = torch.full((B, K), -1000.0)
        hot = torch.arange(B) * 3 % K
        lw[torch.arange(B), hot] = 0.0
        n = torch.full((B, K), T, dtype=torch.int32)
        got = run_spread(lw.cuda(), n.cuda(), where)
        check_spread(got, f64_spread(lw, n, where))
        rows = where.reshape(T, B, K, 4)[:, torch.arange(B), hot]
        assert torch.equal(got["where_mean"], rows) and (got["where_std"] == 0).all() and (got["presence_iw"] == 1).all()
        # equal weights, everybody present: the plain mean and the population standard deviation
        lw = torch.full((B, K), -12.5).cuda()
        got = run_spread(lw, n.cuda(), where)
        check_spread(got, f64_spread(lw, n, where))
        x = where.double().reshape(T, B, K, 4)
        assert (got["where_mean"].double() - x.mean(2)).abs().max() <= 1e-6 * (x.abs().max() + 1)
        assert (got["where_std"].double() - x.std(2, unbiased=False)).abs().max() <= 1e-6 * (x.abs().max() + 1)


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------------
def check_against_plain_entries(ps, out, obs_dev):
    """everything behind the selection must be, bit for bit, what the existing air_parse_objects / air_parse_render give on
    torch-gathered rows of the engine's buffers"""
    eng, B, K, T = ps.engine, ps.B, ps.K, ps.T
    cfg = eng.cfg
    (H, W), (h, w) = cfg.img_size, cfg.crop_size
    ar, ks = torch.arange(B, device=eng.device), out["best_particle"].long()
    pick = lambda x: x.reshape(T, B, K, -1)[:, ar, ks].contiguous()
    where, what, glimpse = pick(eng.where), pick(eng.what), pick(eng.gd.out[-1])
    prob = pick(eng.presence_prob)[..., 0].contiguous()
    n_in = out["num_steps"][ar, ks].contiguous()
    assert torch.equal(out["where"], where) and torch.equal(out["what"], what) and torch.equal(out["presence_prob"], prob)
    assert torch.equal(out["glimpse"].reshape(T, B, -1), glimpse)
    assert torch.equal(out["num_steps_posterior"], eng.q_n.reshape(B, K, T + 1)[:, 0])        # q(n | x) depends on the image alone
    obj = run_objects(prob, n_in, where, what, H, W)
    assert torch.equal(out["num_objects"], n_in)
    total = int(obj["offsets"][-1])
    for k in ("num_objects", "count_prob", "presence", "score", "boxes", "offsets"):
        assert torch.equal(out[k], obj[k]), k
    for k in ("obj_image", "obj_step", "obj_box", "obj_score", "obj_where", "obj_what"):
        assert torch.equal(out[k][:total], obj[k][:total]), k
    ren = run_render(glimpse.reshape(T, B, h, w), where, obj["presence"], obs_dev.reshape(B, -1).contiguous(),
                     float(cfg.output_multiplier), float(cfg.output_std), (H, W), (h, w), layers=ps.layers is not None)
    assert ren["n_bands"] == ps.n_bands
    for k in ("reconstruction", "owner", "area", "rec") + (("layers",) if ps.layers is not None else ()):
        assert torch.equal(out[k], ren[k]), k
    return total


@pytest.mark.parametrize("select", ["joint", "weight"])
@pytest.mark.parametrize("name", ["tiny_b6_k5", "mnist_b8_k8", "rect_t5_b3_k4"])
def test_parse_matches_f64_oracle_under_three_noise_settings(gpu_device, name, select):
    ocfg, B, K = CASES[name]
    T = ocfg.max_steps
    ps = None
    for setting in SETTINGS:
        _, _, _, params, obs, noise, logw, logq, n, res = oracle_case(name, setting)
        if ps is None:
            ps = make_particle_parser(ocfg, B, K, params, select=select, keep_layers=(name == "tiny_b6_k5"))
        ps.engine.set_noise(noise["eps_where"].cuda(), noise["eps_what"].cuda(), noise["u_pres"].cuda())
        out = ps.parse(obs.cuda(), sample_noise=False)
        ps.synchronize()
        assert torch.equal(out["num_steps"].cpu().long(), n)
        assert (out["degenerate"] == 0).all()
        score = logw + logq if select == "joint" else logw                      # [B, K] float64, the oracle's
        m = 2 * OUT_TOL * score.abs().max().item()
        ks = out["best_particle"].cpu().long()
        assert ((ks >= 0) & (ks < K)).all()
        ar = torch.arange(B)
        top = score.max(1).values
        short = top - score[ar, ks]
        top2 = score.sort(1, descending=True).values[:, :2] if K > 1 else None
        gap = top2[:, 0] - top2[:, 1]
        decisive = gap > 2 * m
        print("%s / %s / (%s): m = %.3e, winners %s, oracle argmax %s, worst shortfall %.3e, smallest top-two gap %.3e, %d of %d "
              "images decisive" % (name, select, setting, m, ks.tolist(), score.argmax(1).tolist(), short.max().item(),
                                   gap.min().item(), int(decisive.sum()), B))
        assert (short <= m).all(), (setting, short)                            # every image, none left out
        assert torch.equal(ks[decisive], score.argmax(1)[decisive]), setting
        # the device's own rule on the device's own scores: the smallest k of the class of bit-equal maximal scores
        dev = out["log_weights"].double().cpu() + (out["log_q"].double().cpu() if select == "joint" else 0.0)
        assert torch.equal(dev[ar, ks], dev.max(1).values)
        first = (dev == dev.max(1, keepdim=True).values).double().argmax(1)
        assert torch.equal(ks, first), setting
        assert torch.equal(out["best_score"].cpu(), dev[ar, ks].float())
        total = check_against_plain_entries(ps, out, obs.cuda())
        if setting == "a":                                                      # mixed counts; the n = 0 particles of an image tie exactly
            zero = n == 0
            tied = [b for b in range(B) if zero[b].sum() >= 2]
            assert tied, "no image with two n = 0 particles: the tie rule is not exercised"
            for b in tied:
                idx = zero[b].nonzero().reshape(-1)
                assert (dev[b, idx] == dev[b, idx[0]]).all(), b                 # bit-identical rows, bit-identical scores
        elif setting == "b":                                                    # n = T everywhere: the latents decide, T objects render
            assert (n == T).all() and decisive.all(), (gap, m)                  # the exact assertion covered every image
            assert (out["num_objects"] == T).all() and total == T * B and out["reconstruction"].abs().max() > 0
        else:                                                                   # n = 0 everywhere: every particle ties, the parse is empty
            assert (n == 0).all() and (ks == 0).all() and (out["num_objects"] == 0).all() and total == 0
            assert (out["reconstruction"] == 0).all() and (out["owner"] == -1).all() and (out["area"] == 0).all()
            assert torch.isnan(out["where_mean"]).all() and (out["presence_iw"] == 0).all()
        # the importance-weighted figures are the ones ImportanceEvaluator reports for these weights
        ref = f64_reduce(out["log_weights"], out["num_steps"], T)
        for k, kk in (("iw_bound", "iw_bound"), ("ess", "ess"), ("num_steps_posterior_iw", "num_steps_posterior")):
            assert ((out[k].cpu().double() - ref[kk]).abs() <= 2e-5 * (ref[kk].abs() + 1)).all(), k


# ---- 5. K = 1 at the mode is the deterministic parse ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mnist_b8", "tiny"])
def test_one_particle_at_the_mode_is_the_scene_parse(gpu_device, name):
    ocfg, B, params, obs = e2e_case(name)
    T = ocfg.max_steps
    sp = make_parser(ocfg, B, params, keep_layers=True)
    ref = sp.parse(obs.cuda(), num_objects=T)
    pp = make_particle_parser(ocfg, B, 1, params, mode_noise(ocfg, B), keep_layers=True)
    out = pp.parse(obs.cuda(), sample_noise=False)
    sp.synchronize(); pp.synchronize()
    assert set(ref) <= set(out)
    for k in ref:
        assert ref[k].shape == out[k].shape and torch.equal(ref[k], out[k]), k
    assert (out["best_particle"] == 0).all() and (out["num_steps"] == T).all() and (out["presence_iw"] == 1).all()
    assert torch.equal(out["where_mean"], out["where"]) and (out["where_std"] == 0).all() and (out["ess"] == 1).all()


# ---- 6. graph ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(gpu_device):
    ocfg, B, K = CASES["mnist_b8_k8"]
    params, obs, noise = make_inputs(ocfg, B, K)
    eager = make_particle_parser(ocfg, B, K, params, noise, seed=3)
    graph = make_particle_parser(ocfg, B, K, params, noise, seed=3)
    graph.capture()
    batches = [O.synthetic_batch(ocfg, B, seed=s)[0].cuda() for s in (11, 12)]
    for x in batches:                                              # kept noise: identical bits
        a, b = eager.parse(x, sample_noise=False), graph.parse(x, sample_noise=False)
        eager.synchronize(); graph.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
    kept = []
    for x in (batches[0], batches[0]):                             # fresh particles per call; same seed, same noise state: replay == eager
        a, b = eager.parse(x), graph.parse(x)
        eager.synchronize(); graph.synchronize()
        for k in a:
            assert same_bits(a[k], b[k]), k
        kept.append(b["log_weights"].clone())
    assert not torch.equal(kept[0], kept[1])
    assert graph.launch_count() == {"forward": len(graph.engine._plan_fwd_noise), "rng_advance": 1, "iw": 3, "particle": 2,
                                    "parse_objects": 1, "parse_render": 1, "rec_sum": 1}
    # a run-time switch re-captures: the replayed graph then computes what a parser built with the new value computes
    forced = setting_noise(noise, "b")                             # every particle has T objects: the render is not empty
    for ps in (eager, graph):
        ps.engine.set_noise(forced["eps_where"].cuda(), forced["eps_what"].cuda(), forced["u_pres"].cuda())
    before = graph.parse(batches[1], sample_noise=False)["reconstruction"].clone()
    assert before.abs().max() > 0
    assert graph.update_config(output_multiplier=0.25) and eager.update_config(output_multiplier=0.25)
    assert graph._graphs and set(graph._graphs) == {True, False} and not eager._graphs
    assert not graph.update_config(output_multiplier=0.25)         # nothing changed: nothing rebuilt
    a, b = eager.parse(batches[1], sample_noise=False), graph.parse(batches[1], sample_noise=False)
    eager.synchronize(); graph.synchronize()
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert not torch.equal(b["reconstruction"], before)
    graph.release_graphs()


# ---- 7. model level --------------------------------------------------------------------------------------------------------------
def test_particle_parse_on_the_model_does_not_disturb_training(gpu_device):
    B, T, A, K = 8, 3, 50, 4
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    before = _train_state(air._engine)
    out = air.parse(particles=K)
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air._engine.global_step == 2 and int(air.global_step) == 2
    extra = {"best_particle": (B,), "best_score": (B,), "degenerate": (B,), "log_weights": (B, K), "log_q": (B, K), "num_steps": (B, K),
             "iw_bound": (B,), "ess": (B,), "num_steps_posterior_iw": (B, T + 1), "where_mean": (T, B, 4), "where_std": (T, B, 4),
             "presence_iw": (T, B)}
    shapes = {"num_objects": (B,), "count_prob": (B,), "num_steps_posterior": (B, T + 1), "presence_prob": (T, B), "presence": (T, B),
              "score": (T, B), "boxes": (T, B, 4), "what": (T, B, A), "where": (T, B, 4), "glimpse": (T, B, 20, 20),
              "offsets": (B + 1,), "obj_image": (T * B,), "obj_step": (T * B,), "obj_box": (T * B, 4), "obj_score": (T * B,),
              "obj_where": (T * B, 4), "obj_what": (T * B, A), "reconstruction": (B, 50, 50), "rec": (B,), "owner": (B, 50, 50),
              "area": (T, B)}
    shapes.update(extra)
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes
    assert out is air.parsed and torch.isfinite(out["reconstruction"]).all() and torch.isfinite(out["log_weights"]).all()
    assert ((out["best_particle"] >= 0) & (out["best_particle"] < K)).all() and (out["degenerate"] == 0).all()
    ps = air._particle_parser
    assert ps.K == K and ps.select == "joint" and air.particle_parser(B, K, "joint") is ps
    assert torch.equal(ps.engine.flat_params, air._engine.flat_params) and int(ps.engine.step_dev.item()) == 2
    # the deterministic path is untouched by the particle parser's existence
    det = air.parse()
    assert "best_particle" not in det and air._scene_parser is not None and air._particle_parser is ps
    assert air.particle_parser(B, K, "weight") is not ps           # another criterion: another parser
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # the logger: the deterministic keys + the two particle figures
    from attend_infer_repeat_amd.evaluation import make_parse_logger
    got = make_parse_logger(air, lambda: (x, y), 2, "test", particles=K)(itr=3)
    assert set(got) == {"map_num_step_acc", "count_prob", "num_objects", "best_particle_moved", "ess"}
    assert 0.0 <= got["best_particle_moved"] <= 1.0 and 1 - 1e-4 <= got["ess"] <= K + 1e-3
    with pytest.raises(ValueError, match="num_objects together with particles"):
        air.parse(num_objects=2, particles=K)


def test_score_parse_with_particles(gpu_device):
    B, K, G = 8, 4, 2
    air, ts, x, y = _mnist_air(B)
    ts()
    rng = np.random.default_rng(3)
    inst = np.full((B, 50, 50), -1, np.int8)
    boxes = np.zeros((B, G, 4), np.float32)
    for b in range(B):
        for j in range(int(rng.integers(0, G + 1))):
            l, t, w, h = (int(v) for v in (rng.integers(0, 30), rng.integers(0, 30), rng.integers(5, 20), rng.integers(5, 20)))
            inst[b, t:t + h, l:l + w] = j
            boxes[b, j] = (l, t, w, h)
    gt_count = torch.from_numpy((boxes[..., 2] > 0).sum(1)).int()
    scores = air.score_parse(x, torch.from_numpy(inst), torch.from_numpy(boxes), particles=K)
    assert scores is air.parse_scores and "best_particle" in air.parsed
    scorer = air.parse_scorer(G, particles=K)
    assert scorer is air._parse_scorer and scorer.parser is air._particle_parser and scorer.R == B
    diff = air.parsed["num_objects"].cpu().long() - gt_count.long()                  # (the scorer keeps the sign: DESIGN 11)
    assert torch.equal(scores["count_err"].cpu().long(), diff) and torch.equal(scores["count_err"].cpu().long().abs(), diff.abs())
    summ = scorer.summary()
    assert summ["images"] == B and 0.0 <= summ["count_acc"] <= 1.0
    # the logger walks an annotated set, names K and the criterion in its line
    from attend_infer_repeat_amd.evaluation import make_parse_score_logger
    data = dict(imgs=x.cpu().numpy(), boxes=boxes, instances=inst)
    got = make_parse_score_logger(air, data, 1, "test", particles=K, select="weight")(itr=1)
    assert got["images"] == B and 0.0 <= got["best_particle_moved"] <= 1.0 and 1 - 1e-4 <= got["ess"] <= K + 1e-3
    assert air._parse_scorer.parser.select == "weight"
    # without particles the scorer goes back to the deterministic parser
    air.score_parse(x, torch.from_numpy(inst), torch.from_numpy(boxes))
    assert air._parse_scorer.parser is air._scene_parser and "best_particle" not in air.parsed


def test_training_script_parse_particles_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--parse-eval",
                            "--parse-particles", "4"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse(4, joint) ") == 2
    for l in rec:
        assert l["particles"] == 4 and l["select"] == "joint"
        assert 0.0 <= l["map_num_step_acc"] <= 1.0 and 0.0 < l["count_prob"] <= 1.0 and 0.0 <= l["num_objects"] <= 3.0
        assert 0.0 <= l["best_particle_moved"] <= 1.0 and 1 - 1e-4 <= l["ess"] <= 4 + 1e-3


def test_bf16_throughput_plan(gpu_device):
    """mnist_b16_k64: 1024 rows, the throughput plan, bf16 operands"""
    name = "mnist_b16_k64"
    ocfg, B, K = CASES[name]
    params, obs, noise = make_inputs(ocfg, B, K)
    with O.matmul_mode("bf16"):
        _, _, res = oracle_log_weights(ocfg, params, obs, noise, K, True)
        noise, moved = _separate_borderline_draws(noise, res)
        _, n, res = oracle_log_weights(ocfg, params, obs, noise, K, True)
        logq = oracle_log_q(ocfg, res, n)
    ps = make_particle_parser(ocfg, B, K, params, noise, mfma_dtype="bf16")
    out = ps.parse(obs.cuda(), sample_noise=False)
    ps.synchronize()
    assert ps.engine.cfg.mfma_dtype == "bf16"
    assert torch.equal(out["num_steps"].cpu().reshape(-1).long(), n.long())
    for k, v in out.items():
        if v.dtype.is_floating_point and k not in ("where_mean", "where_std"):
            assert torch.isfinite(v[:int(out["offsets"][-1])] if k.startswith("obj_") else v).all(), k
    has = out["presence_iw"] > 0                                    # a step somebody has: its spread is a number
    assert torch.isfinite(out["where_mean"][has]).all() and torch.isfinite(out["where_std"][has]).all()
    assert ((out["best_particle"] >= 0) & (out["best_particle"] < K)).all() and (out["degenerate"] == 0).all()
    err = rel_err(out["log_q"].reshape(-1), logq)
    print("bf16 log q: worst / max = %.3e (%d borderline draws moved)" % (err, moved))
    assert err < 2e-3, err
    check_against_plain_entries(ps, out, obs.cuda())
