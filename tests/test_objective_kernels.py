"""GPU parity of the objective-side kernels, one kernel at a time (run with -m gpu on an MI355X): presence, the count posterior q(n)
with its KL / step weights / log q(n*) in the generic and the fused (<8> and <32>) forms up to T = 32, NVIL with its moving-average
block and its shares, the importance weight, the reconstruction term, the baseline packing and the prior table.

References are float64: the functions of oracle/air_oracle.py, or the few lines written out in the test.  Inputs are built so that
no comparison has to leave an element out; every such condition (the margin of u around p, the margin of sum_t p around an
integer, the column whose sampled count sits on a clamped q(n)) is asserted where the input is made.

Group letters (A count posterior, B NVIL / importance weight, C presence / reconstruction / packing / prior) tag every comparison;
the worst error / tolerance ratio of each group is printed when the module finishes (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from oracle import air_oracle as O

from attend_cases import (BWD_VARIANTS, KL_SCALE, NSP, W_SCALE, _check_fused_forward, _margin_u, _objective64, _posterior_refs,
                          _presence_prob64, assert_bits, assert_close, g, print_worst)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print_worst("objective kernels", "ABC")


# ---------------------------------------------------------------------------------------------------------------
# A. count posterior, generic and fused, up to T = 32
# ---------------------------------------------------------------------------------------------------------------
# every T at B = 130 (three blocks of the fused form, one of the generic), every B at the T == MT edge (8), the first <32> size (9) and 32
TB_CASES = [(T, 130) for T in (1, 5, 8, 9, 16, 32)] + [(T, B) for T in (8, 9, 32) for B in (1, 63, 65)]


def _assert_clamp_column(p64, pres, T, clamped, q32=None):
    """column 1: presence forced to all ones, so that the sampled count T sits on q(T) = prod_t p_t"""
    assert bool((pres[:, 1] == 1).all()) and int(pres[:, 1].sum()) == T
    q64 = O.bernoulli_to_modified_geometric(p64.t())
    if clamped:
        assert float(q64[1, T]) <= 1e-32, f"q(T) = {float(q64[1, T]):.3e} is above the clamp"
    if q32 is not None and T == 32:
        assert float(q32[1, T]) == 0.0                                          # underflows in float32


@functools.lru_cache(maxsize=None)
def _generic_case(T, B):
    gen = torch.Generator().manual_seed(1000 * T + B)
    prob = torch.rand(T, B, generator=gen) * 0.98 + 0.01
    z = (torch.rand(T, B, generator=gen) < prob).float()
    if B > 1:                                                                   # B = 1: an ordinary column
        prob[:, 0] = 1.0 - 1e-4; prob[:, 1] = 1e-4
        z[:, 1] = 1.0
    pres = torch.cumprod(z, 0)
    prior = O.geometric_prior(NSP, T)
    q, kl, w, logp = _posterior_refs(prob, pres.sum(0), prior)
    if B > 1:
        _assert_clamp_column(prob.double(), pres, T, T >= 8, q)
    dw = torch.randn(T, B, generator=gen); dl = torch.randn(B, generator=gen)
    p64 = prob.double().requires_grad_(True)
    gp, = torch.autograd.grad(_objective64(p64, pres.sum(0), prior, 0.37, dw, dl), [p64])
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(logp).all())
    return dict(prob=prob, pres=pres, prior=prior, q=q, kl=kl, w=w, logp=logp, dw=dw, dl=dl, dprob=gp)


@pytest.mark.parametrize("T,B", TB_CASES)
def test_numsteps_generic_up_to_32_steps(hip, T, B):
    c = _generic_case(T, B)
    prob, pres, prior = c["prob"].cuda(), c["pres"].cuda(), c["prior"].cuda()
    qg, klg, logpg, wg = hip.numsteps_fwd(prob, pres, prior)
    tag = f"numsteps_fwd T={T} B={B} "
    assert_close(qg, c["q"], 1e-6, 1e-8, tag + "q", "A"); assert_close(klg, c["kl"], 1e-5, 1e-6, tag + "kl", "A")
    assert_close(wg, c["w"], 1e-6, 1e-7, tag + "w", "A"); assert_close(logpg, c["logp"], 1e-5, 1e-6, tag + "logp", "A")
    dprob = hip.numsteps_bwd(prob, pres, prior, 0.37, c["dw"].cuda(), c["dl"].cuda())
    assert_close(dprob, c["dprob"], 2e-4, 2e-4, f"numsteps_bwd T={T} B={B} dprob", "A")


@functools.lru_cache(maxsize=None)
def _fused_case(T, B, step_bias, eps, continuous=False):
    """logits (randn * 3) with, for B > 1 on the discrete path, column 0 at p ~ 1 - 1e-4 and column 1 at p ~ 1e-4 with its presence
    forced to ones; the float64 chain sigmoid -> eps mix -> Bernoulli cumprod -> count"""
    gen = torch.Generator().manual_seed(7919 * T + 13 * B + (1 if eps is None else 0) + (2 if step_bias else 0) + (4 if continuous else 0))
    logit = torch.randn(T, B, generator=gen) * 3
    if continuous:
        # the count is int(sum_t p): keep the sum at least 0.05 away from an integer, so that the order of a float32 sum cannot move it
        for _ in range(200):
            frac = torch.remainder(_presence_prob64(logit.double(), step_bias, eps).sum(0), 1.0)
            bad = (frac < 0.05) | (frac > 0.95)
            if not bool(bad.any()):
                break
            logit[:, bad] = torch.randn(T, int(bad.sum()), generator=gen) * 3
        p64 = _presence_prob64(logit.double(), step_bias, eps)
        frac = torch.remainder(p64.sum(0), 1.0)
        assert bool(((frac >= 0.05) & (frac <= 0.95)).all())
        return dict(logit=logit, u=None, p64=p64, pres=p64, count=torch.floor(p64.sum(0)))
    if B > 1:
        logit[:, 0] = 9.2 - step_bias; logit[:, 1] = -9.3 - step_bias
    p64 = _presence_prob64(logit.double(), step_bias, eps)
    u = torch.rand(T, B, generator=gen)
    if B > 1:
        u[:, 1] = 0.0                                                           # u < p at every step: the chain stays 1
    u = _margin_u(u, p64)
    pres = torch.cumprod((u.double() < p64).double(), 0)
    if B > 1:
        # p ~ 9.1e-5 without the eps mix, ~ 5.9e-4 with it: prod_t p is below 1e-32 from T = 8 and from T = 16
        _assert_clamp_column(p64, pres, T, (eps is None and T >= 8) or T >= 16)
    return dict(logit=logit, u=u, p64=p64, pres=pres, count=pres.sum(0))


@pytest.mark.parametrize("explore_eps", [1e-3, None])
@pytest.mark.parametrize("step_bias", [0.0, 0.75])
@pytest.mark.parametrize("T,B", TB_CASES)
def test_presence_numsteps_fwd(hip, T, B, step_bias, explore_eps):
    c = _fused_case(T, B, step_bias, explore_eps)
    prior = O.geometric_prior(NSP, T)
    out = hip.presence_numsteps_fwd(c["logit"].cuda(), c["u"].cuda(), step_bias, explore_eps, prior.cuda())
    _check_fused_forward(out, c, prior, f"presence_numsteps_fwd T={T} B={B} bias={step_bias} eps={explore_eps} ")


@pytest.mark.parametrize("step_bias,explore_eps", [(0.75, 1e-3), (0.0, None)])
@pytest.mark.parametrize("T,B", TB_CASES)
def test_presence_numsteps_fwd_continuous_steps(hip, T, B, step_bias, explore_eps):
    c = _fused_case(T, B, step_bias, explore_eps, continuous=True)
    prior = O.geometric_prior(NSP, T)
    out = hip.presence_numsteps_fwd(c["logit"].cuda(), None, step_bias, explore_eps, prior.cuda())
    _check_fused_forward(out, c, prior, f"presence_numsteps_fwd (u = None) T={T} B={B} bias={step_bias} eps={explore_eps} ")


@functools.lru_cache(maxsize=None)
def _bwd_case(T, B, variant):
    name, continuous, has_a, has_b, has_dlogp, has_dpres, step_bias, eps = BWD_VARIANTS[variant]
    c = _fused_case(T, B, step_bias, eps, continuous)
    gen = torch.Generator().manual_seed(31 * T + B + 1009 * variant)
    ka = torch.rand(T, B, generator=gen) * 4 if has_a else None
    kb = torch.rand(T, B, generator=gen) * 40 if has_b else None
    dlogp = torch.randn(B, generator=gen) if has_dlogp else None
    dpres = torch.randn(T, B, generator=gen) if has_dpres else None
    prior = O.geometric_prior(NSP, T)
    l64 = c["logit"].double().requires_grad_(True)
    p = _presence_prob64(l64, step_bias, eps)
    dw = None
    if has_a or has_b:
        dw = W_SCALE * ((ka.double() if has_a else 0.0) + (kb.double() if has_b else 0.0))
    L = _objective64(p, c["count"], prior, KL_SCALE, dw, dlogp)
    if has_dpres:
        L = L + (dpres.double() * p).sum()
    gl, = torch.autograd.grad(L, [l64])
    assert bool(torch.isfinite(gl).all())
    prob32 = c["p64"].float()
    return dict(c, prob=prob32, presence=prob32 if continuous else c["pres"].float(), ka=ka, kb=kb, dlogp=dlogp, dpres=dpres, prior=prior,
                dlogit=gl, name=name, continuous=continuous, step_bias=step_bias, eps=eps)


def _fused_bwd_args(c):
    return (g(c["prob"]), g(c["presence"]), c["prior"].cuda(), KL_SCALE, g(c["ka"]), g(c["kb"]), W_SCALE, g(c["dlogp"]), g(c["dpres"]),
            g(c["logit"]), c["step_bias"], c["eps"])


@pytest.mark.parametrize("T,B", TB_CASES)
def test_numsteps_presence_bwd(hip, T, B):
    for variant in range(len(BWD_VARIANTS)):
        c = _bwd_case(T, B, variant)
        tag = f"numsteps_presence_bwd T={T} B={B} [{c['name']}] "
        args = _fused_bwd_args(c)
        dlogit = hip.numsteps_presence_bwd(*args)
        assert_close(dlogit, c["dlogit"], 2e-4, 2e-4, tag + "against float64 autograd", "A")
        # the unfused composition of include/air_hip.h: dstep_weight = w_scale * (kl_a + kl_b) -> air_numsteps_bwd -> air_presence_bwd
        prob, presence, prior, _, ka, kb, _, dlogp, dpres, logit, _, _ = args
        dstep = None
        if ka is not None or kb is not None:
            dstep = W_SCALE * ((ka if ka is not None else 0.0) + (kb if kb is not None else 0.0))
        dprob = hip.numsteps_bwd(prob, presence, prior, KL_SCALE, dstep, dlogp)
        unfused = hip.presence_bwd(logit, c["step_bias"], c["eps"], not c["continuous"], dprob, dpres)
        assert_close(dlogit, unfused, 2e-4, 2e-4, tag + "against numsteps_bwd + presence_bwd", "A")


GAUSS_PRIOR4, GAUSS_OFF = (0.3, 1.5, -0.2, 0.7), 0.5


@pytest.mark.parametrize("T", [5, 9, 32])
def test_heads_equal_their_two_halves_bit_for_bit(hip, T):
    """air_heads_fwd / _bwd run the Gaussian body and the <MT> count body in one launch, blocks split by role: each half must give
    the bits of its stand-alone launch (a wrong split of the grid or a missing tail of rows / columns shows here)."""
    B, D = 65, 4
    M = T * B
    gen = torch.Generator().manual_seed(100 + T)
    pre = (torch.randn(M, 2 * D + 3, generator=gen) * 2).cuda()[:, :2 * D]      # row stride 2D + 3
    eps = torch.randn(M, D, generator=gen).cuda()
    dsample = torch.randn(M, D, generator=gen).cuda(); dkl = torch.randn(M, generator=gen).cuda()
    c = _bwd_case(T, B, 0)
    logit, u, prior = c["logit"].cuda(), c["u"].cuda(), c["prior"].cuda()
    gauss, count = hip.heads_fwd(pre, eps, GAUSS_OFF, 1, GAUSS_PRIOR4, logit, u, c["step_bias"], c["eps"], prior)
    for got, ref, nm in zip(gauss, hip.gauss_sample_fwd(pre, eps, GAUSS_OFF, 1, GAUSS_PRIOR4), ("loc", "scale", "sample", "kl_row")):
        assert_bits(got, ref, f"heads_fwd T={T} {nm}")
    alone = hip.presence_numsteps_fwd(logit, u, c["step_bias"], c["eps"], prior)
    for got, ref, nm in zip(count, alone, ("prob", "presence", "q", "kl", "logp", "step_weight")):
        assert_bits(got, ref, f"heads_fwd T={T} {nm}")
    _check_fused_forward(count, c, c["prior"], f"heads_fwd T={T} B={B} ")
    loc, scale = gauss[0], gauss[1]
    for variant in (0, 4):                                                      # the discrete and the continuous path (dpresence)
        c = _bwd_case(T, B, variant)
        args = _fused_bwd_args(c)
        dpre, dlogit = hip.heads_bwd(pre, eps, GAUSS_OFF, 1, GAUSS_PRIOR4, loc, scale, dsample, dkl, *args)
        assert_bits(dpre, hip.gauss_sample_bwd(pre, eps, GAUSS_OFF, 1, GAUSS_PRIOR4, loc, scale, dsample, dkl), f"heads_bwd T={T} dpre")
        assert_bits(dlogit, hip.numsteps_presence_bwd(*args), f"heads_bwd T={T} dlogit [{c['name']}]")
        assert_close(dlogit, c["dlogit"], 2e-4, 2e-4, f"heads_bwd T={T} dlogit [{c['name']}] against float64 autograd", "A")


# ---------------------------------------------------------------------------------------------------------------
# B. NVIL and the importance weight
# ---------------------------------------------------------------------------------------------------------------
NVIL_B = [1, 2, 63, 64, 65, 257, 1100]      # one lane, a part of / exactly / just over one pass of wave 0, over the 256 threads, many passes


def _nvil_inputs(B, kind, seed=9):
    gen = torch.Generator().manual_seed(seed + B)
    imp = torch.rand(B, generator=gen) * 3000 + 500; base = torch.randn(B, generator=gen) * 10
    logp = -torch.rand(B, generator=gen) * 3
    if kind in ("equal_imp", "zero_variance"):
        imp = torch.full((B,), 2000.0)
    if kind == "zero_variance":
        base = torch.full((B,), 7.5)
    if kind == "offset":                                                        # the magnitude at 100x100 images: E[x^2] - E[x]^2 cancels
        imp = 6e4 + torch.randn(B, generator=gen)
    return imp, base, logp


def _nvil_ref(imp, base, logp, ema=None):
    """the [B, B] broadcast in float64, as in test_nvil; ema = (moving_mean, moving_var) as they stand before the step"""
    b64 = base.double().requires_grad_(True); l64 = logp.double().requires_grad_(True)
    raw = imp.double()[None, :] - b64[:, None]                                  # (i, j) = imp_j - b_i
    iw = raw if ema is None else (raw - ema[0]) / max(float(np.sqrt(ema[1])), 1.0)
    rl = (iw.detach() * l64).mean(); bl = 0.5 * (raw ** 2).mean()               # the baseline loss is not normalised
    gl, = torch.autograd.grad(rl, [l64]); gb, = torch.autograd.grad(bl, [b64])
    out = torch.stack([rl.detach(), bl.detach(), iw.mean().detach(), iw.var(unbiased=False).detach()])
    return out, gl, gb, raw.detach().mean(), raw.detach().var(unbiased=False)


def _check_nvil(got, ref, tag, rtol_only_baseline_loss=False, group="B"):
    out, dlogp, dbase = got
    rout, rdlogp, rdbase = ref
    assert bool(torch.isfinite(out).all())
    if rtol_only_baseline_loss:                                                 # out[1] ~ 1.8e9: an absolute 1e-3 means nothing there
        keep = torch.tensor([0, 2, 3])
        assert_close(out.cpu()[keep], rout[keep], 1e-5, 1e-3, tag + "scalars 0, 2, 3", group)
        assert_close(out.cpu()[1:2], rout[1:2], 1e-5, 0.0, tag + "baseline loss", group)
    else:
        assert_close(out, rout, 1e-5, 1e-3, tag + "scalars", group)
    assert_close(dlogp, rdlogp, 1e-5, 1e-5, tag + "dlogp", group); assert_close(dbase, rdbase, 1e-5, 1e-5, tag + "dbaseline", group)


@pytest.mark.parametrize("kind", ["plain", "equal_imp", "zero_variance", "offset"])
@pytest.mark.parametrize("B", NVIL_B)
def test_nvil_batch_sizes_and_magnitudes(hip, B, kind):
    imp, base, logp = _nvil_inputs(B, kind)
    ref = _nvil_ref(imp, base, logp)
    got = hip.nvil(imp.cuda(), base.cuda(), logp.cuda())
    _check_nvil(got, ref[:3], f"nvil B={B} {kind} ", rtol_only_baseline_loss=(kind == "offset"))
    if kind == "zero_variance":
        assert abs(float(got[0][3])) <= 1e-3


@pytest.mark.parametrize("moving_var,decay,update", [(0.25, 0.99, 1), (9.0, 0.8, 1), (0.25, 0.8, 0), (9.0, 0.99, 0)])
@pytest.mark.parametrize("B", NVIL_B)
def test_nvil_moving_average_block(hip, B, moving_var, decay, update):
    imp, base, logp = _nvil_inputs(B, "plain", seed=21)
    batch_mean = float((imp.double().mean() - base.double().mean()))
    block = torch.tensor([0.5 * batch_mean, moving_var, decay, float(update)], dtype=torch.float32)
    mm, mv, d = (float(v) for v in block[:3])                                   # what the kernel is given: the float32 values
    rout, rdlogp, rdbase, raw_mean, raw_var = _nvil_ref(imp, base, logp, ema=(mm, mv))
    ema = block.cuda()
    got = hip.nvil(imp.cuda(), base.cuda(), logp.cuda(), ema)
    tag = f"nvil ema B={B} var={moving_var} decay={decay} update={update} "
    _check_nvil(got, (rout, rdlogp, rdbase), tag)                               # normalised by the values from BEFORE the update
    if update:
        assert_close(ema[:2], torch.stack([d * mm + (1 - d) * raw_mean, d * mv + (1 - d) * raw_var]), 1e-5, 0.0, tag + "averages", "B")
        assert_bits(ema[2:].cpu(), block[2:], tag + "decay, update")
    else:
        assert_bits(ema.cpu(), block, tag + "block of a read-only pass")


@pytest.mark.parametrize("n_parts", [1, 3])
@pytest.mark.parametrize("B", NVIL_B)
def test_nvil_parts_equals_nvil_on_the_share_sum(hip, B, n_parts):
    gen = torch.Generator().manual_seed(50 + B + n_parts)
    _, base, logp = _nvil_inputs(B, "plain", seed=33)
    parts = torch.rand(n_parts, B, generator=gen) * torch.tensor([2000.0, 300.0, 40.0])[:n_parts, None] + 7.0
    total = parts[0].clone()
    for p in range(1, n_parts):
        total = total + parts[p]                                                # float32, in share order
    for with_ema in (False, True):
        block = torch.tensor([800.0, 9.0, 0.9, 1.0])
        ema_a, ema_b = (block.cuda(), block.cuda()) if with_ema else (None, None)
        out, dlogp, dbase, imp_sum = hip.nvil_parts(parts.cuda(), base.cuda(), logp.cuda(), ema_a)
        tag = f"nvil_parts B={B} n_parts={n_parts} ema={with_ema} "
        assert_bits(imp_sum, total, tag + "imp_sum")
        rout, rdlogp, rdbase = hip.nvil(imp_sum, base.cuda(), logp.cuda(), ema_b)
        assert_bits(out, rout, tag + "out"); assert_bits(dlogp, rdlogp, tag + "dlogp"); assert_bits(dbase, rdbase, tag + "dbaseline")
        if with_ema:
            assert_bits(ema_a, ema_b, tag + "moving averages")
            assert not torch.equal(ema_a.cpu(), block)
    _check_nvil((out, dlogp, dbase), _nvil_ref(total, base, logp, ema=(800.0, 9.0))[:3], f"nvil_parts B={B} n_parts={n_parts} ")


@pytest.mark.parametrize("B", [65, 600])
@pytest.mark.parametrize("T", [1, 5, 9])
@pytest.mark.parametrize("n_parts", [1, 3])
def test_imp_weight(hip, n_parts, T, B):
    gen = torch.Generator().manual_seed(977 * n_parts + 31 * T + B)
    parts = torch.rand(n_parts, B, generator=gen) * torch.tensor([2000.0, 300.0, 40.0])[:n_parts, None] + 7.0
    kl_n = torch.rand(B, generator=gen) * 3; ka = torch.rand(T, B, generator=gen) * 2; kb = torch.rand(T, B, generator=gen) * 0.5
    w = torch.rand(T, B, generator=gen); before = torch.randn(T, B, generator=gen)
    nsp_w, dkl_scale = 0.7, 0.37
    total = parts[0].clone()
    for p in range(1, n_parts):
        total = total + parts[p]
    for use_n in (True, False):
        for use_a in (True, False):
            for use_b in (True, False):
                kl_rows = (ka.double() if use_a else 0.0) + (kb.double() if use_b else torch.zeros(T, B, dtype=torch.float64))
                imp64 = parts.double().sum(0) + (nsp_w * kl_n.double() if use_n else 0.0) + (w.double() * kl_rows).sum(0)
                for want_imp, want_dpres in ((True, True), (True, False), (False, True)):
                    tag = f"imp_weight n_parts={n_parts} T={T} B={B} kl_n={use_n} kl_a={use_a} kl_b={use_b} imp={want_imp} dpres={want_dpres} "
                    dpres = before.cuda() if want_dpres else None
                    rec, imp = hip.imp_weight(parts.cuda(), w.cuda(), g(kl_n) if use_n else None, nsp_w, g(ka) if use_a else None,
                                              g(kb) if use_b else None, want_imp, dpres, dkl_scale)
                    assert_bits(rec, total, tag + "rec")
                    assert (imp is not None) == want_imp
                    if want_imp:
                        assert_close(imp, imp64, 1e-6, 0.0, tag + "imp", "B")
                    if want_dpres:
                        assert_close(dpres.cpu().double() - before.double(), dkl_scale * kl_rows, 1e-6, 1e-6, tag + "dpresence increment", "B")


# ---------------------------------------------------------------------------------------------------------------
# C. presence, reconstruction, packing, prior table
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(3, 300), (1, 1), (3, 1), (2, 2100)])            # one column, one block with a tail, nine blocks with a tail
def test_presence_fwd_with_presence_in(hip, T, B):
    gen = torch.Generator().manual_seed(17 * T + B)
    logit = torch.randn(T, B, generator=gen) * 2
    p64 = _presence_prob64(logit.double(), 0.75, 1e-3)
    u = _margin_u(torch.rand(T, B, generator=gen), p64)
    pin = (torch.rand(B, generator=gen) < 0.7).float()
    if B > 1:
        pin[0] = 0.0; pin[1] = 1.0
    for presence_in in (pin, torch.zeros(B), None):
        start = torch.ones(B, dtype=torch.float64) if presence_in is None else presence_in.double()
        pres = torch.cumprod((u.double() < p64).double(), 0) * start[None]
        prob, pr = hip.presence_fwd(logit.cuda(), u.cuda(), 0.75, 1e-3, True, g(presence_in))
        assert_close(prob, p64, 1e-6, 1e-7, f"presence_fwd T={T} B={B} prob", "C")
        assert torch.equal(pr.cpu().double(), pres), f"presence_fwd T={T} B={B} presence"
        if presence_in is not None:
            assert bool((pr.cpu()[:, presence_in == 0] == 0).all())                 # a chain that starts at 0 stays 0


@pytest.mark.parametrize("T,B", [(3, 300), (1, 1), (5, 2100)])
def test_presence_bwd_options(hip, T, B):
    gen = torch.Generator().manual_seed(23 * T + B)
    logit = torch.randn(T, B, generator=gen) * 2
    dprob = torch.randn(T, B, generator=gen); dpres = torch.randn(T, B, generator=gen)
    # discrete, dprob, dpres, step_bias, explore_eps
    for discrete, has_dprob, has_dpres, bias, eps in [(False, True, True, 0.75, 1e-3), (False, False, True, 0.0, None),
                                                      (True, True, True, 0.75, None), (True, True, False, 0.0, 1e-3),
                                                      (True, False, False, 0.75, 1e-3)]:
        l64 = logit.double().requires_grad_(True)
        p = _presence_prob64(l64, bias, eps)
        L = (p * 0.0).sum()
        if has_dprob:
            L = L + (p * dprob.double()).sum()
        if has_dpres and not discrete:                                          # the sampled presence of the discrete path carries no gradient
            L = L + (p * dpres.double()).sum()
        gl, = torch.autograd.grad(L, [l64])
        got = hip.presence_bwd(logit.cuda(), bias, eps, discrete, g(dprob) if has_dprob else None, g(dpres) if has_dpres else None)
        assert_close(got, gl, 1e-4, 1e-6, f"presence_bwd T={T} B={B} discrete={discrete} dprob={has_dprob} dpres={has_dpres} eps={eps}", "C")


# (2100, 251): more images than the 2048 blocks of the forward, and 2100 * 251 > 2048 * 256 elements, so both grid-stride loops wrap
@pytest.mark.parametrize("B,P", [(1, 1), (3, 255), (5, 257), (2100, 251)])
def test_rec_loglik_shapes(hip, B, P):
    gen = torch.Generator().manual_seed(5 + B + P)
    obs = torch.rand(B, P, generator=gen); canvas = torch.randn(B, P, generator=gen)
    dps = torch.rand(B, generator=gen) * 0.5 + 0.1
    mult, std = 0.5, 0.3
    c64 = canvas.double().requires_grad_(True)
    nll = (0.5 * ((obs.double() - mult * c64) / std) ** 2 + 0.5 * np.log(2 * np.pi) + np.log(std)).sum(1)
    assert_close(hip.rec_loglik_fwd(obs.cuda(), canvas.cuda(), mult, std), nll, 1e-5, 1e-6 * P, f"rec_loglik_fwd B={B} P={P}", "C")
    gc, = torch.autograd.grad(nll.mean(), [c64], retain_graph=True)
    assert_close(hip.rec_loglik_bwd(obs.cuda(), canvas.cuda(), mult, std, None, 1.0 / B), gc, 1e-5, 1e-6, f"rec_loglik_bwd B={B} P={P} uniform", "C")
    gd, = torch.autograd.grad((nll * dps.double()).sum(), [c64])
    assert_close(hip.rec_loglik_bwd(obs.cuda(), canvas.cuda(), mult, std, dps.cuda(), 123.0), gd, 1e-5, 1e-6,
                 f"rec_loglik_bwd B={B} P={P} dper_sample", "C")


@pytest.mark.parametrize("T,B,hw,A,states", [(3, 210, 50, 50, (256, 256)),      # 210 * 3177 > 2048 * 256: the element loop wraps
                                             (3, 5, 50, 50, (256,)), (2, 7, 9, 3, ()), (1, 1, 1, 1, (1, 2))])
def test_baseline_pack_sizes_and_state_parts(hip, T, B, hw, A, states):
    gen = torch.Generator().manual_seed(2 + B)
    obs = torch.rand(B, hw, hw, generator=gen); what = torch.randn(T, B, A, generator=gen)
    where = torch.randn(T, B, 4, generator=gen); pres = torch.rand(T, B, 1, generator=gen)
    parts = [torch.randn(B, s, generator=gen) for s in states]
    ref = torch.cat([obs.reshape(B, -1)] + [t.permute(1, 0, 2).reshape(B, -1) for t in (what, where, pres)] + parts, -1)
    if B == 210:
        assert ref.numel() > 2048 * 256
    out = hip.baseline_pack(obs.cuda(), what.cuda(), where.cuda(), pres.cuda(), [s.cuda() for s in parts])
    assert torch.equal(out.cpu(), ref)


PRIOR_CASES = [
    # anneal_type, init, final, anneal_steps, hold_for, steps_div, global steps
    (None, 0.3, 0.0, 1.0, 0.0, 1.0, (0, 12345)),
    ("exp", 1.0 - 1e-5, 1e-5, 1e5, 1e3, 1e4, (0, 999, 1000, 40_000, 10_000_000)),   # before the hold, its end, the middle, far past the end
    ("linear", 1.0 - 1e-5, 1e-5, 1e5, 1e3, 1.0, (0, 999, 1000, 40_000, 10_000_000)),
    (None, 0.0, 0.0, 1.0, 0.0, 1.0, (0,)),                                          # below the clip: 1e-7
    (None, 1e-7, 0.0, 1.0, 0.0, 1.0, (0,)),
    (None, 1.0, 0.0, 1.0, 0.0, 1.0, (0,)),                                          # above the clip: 1 - 1e-15
    (None, 1.0 - 1e-15, 0.0, 1.0, 0.0, 1.0, (0,)),
    ("linear", 1.0, 0.0, 50.0, 0.0, 1.0, (0, 25, 50, 51)),                          # both ends of the annealing lie outside the clip
]


@pytest.mark.parametrize("T", [1, 5, 32])
@pytest.mark.parametrize("case", range(len(PRIOR_CASES)))
def test_steps_prior_table(hip, case, T):
    anneal, init, final, steps, hold, div, global_steps = PRIOR_CASES[case]
    for step in global_steps:
        s = init if anneal is None else O.anneal_weight(init, final, anneal, step, steps, hold, div)
        ref = O.geometric_prior(s, T)
        assert bool(torch.isfinite(ref).all()) and ref.shape == (T + 1,)
        got = hip.steps_prior(torch.tensor([step], dtype=torch.int64).cuda(), T, init, final, anneal, steps, hold, div)
        assert got.dtype == torch.float64
        assert_close(got, ref, 1e-12, 0.0, f"steps_prior T={T} case={case} step={step}", "C")
