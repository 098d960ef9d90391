"""GPU tests of training on the K-particle importance-weighted bound (csrc/iw_train_kernels.hip, functional.iw_logweight / vimco,
AIRModel.train_step(iw_samples=K)): the two entries against their host restatements (iw_train.py), the autograd pair against a
float64 restatement in torch, one update end to end on the tiny golden model, and the public surface.

Bars.  air_iw_logweight_bwd is element-wise float32 without contraction: bit for bit against reference_logweight_grad.  air_iw_vimco
computes in float64 and rounds once: one float32 ulp of the reference, or 2^-40 * max(1, |bound|) absolutely (the cancellation in
bound - bound-without-k) where that is larger.  The autograd gradients are a coefficient within one float32 ulp times an element-wise
derivative within a few: 2^-18 of each tensor's largest element."""
import json
import os

import numpy as np
import pytest
import torch

from attend_infer_repeat_amd import iw_train as IT
from oracle import air_oracle as O
from test_iw_train_host import NAMES, PRIORS, logweight_inputs

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = 3


def same_bits(got, ref):
    """equal as bits, a NaN of any payload equal to a NaN"""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return bool(((got.view(np.int32) == ref.view(np.int32)) | (np.isnan(got) & np.isnan(ref))).all())


# ---- air_iw_logweight_bwd ------------------------------------------------------------------------------------------------------------
OUT_SHAPES = lambda R, A: [(T, R, A)] * 3 + [(T, R, 4)] * 3 + [(R,)] * 2


def run_logweight_bwd(a, A, priors):
    """the entry through the C ABI on output buffers filled with NaN: a row the kernel does not write shows"""
    from attend_infer_repeat_amd import _lib, hip as H
    R = a["g"].shape[0]
    dev = {k: torch.from_numpy(np.ascontiguousarray(a[k])).cuda() for k in NAMES + ("presence", "g")}
    outs = [torch.full(s, float("nan"), device="cuda") for s in OUT_SHAPES(R, A)]
    st = H.lib().air_iw_logweight_bwd(*[H._p(dev[k]) for k in NAMES + ("presence", "g")], T, R, 1, A, *[float(v) for v in priors],
                                      *[H._p(o) for o in outs], H._stream())
    _lib.check(st, "air_iw_logweight_bwd")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("form", list(PRIORS))
@pytest.mark.parametrize("A", [50, 6, 5, 8])                       # V = 2, 2, 1, 4
def test_logweight_bwd_is_the_host_restatement_bit_for_bit(gpu_device, A, form):
    pr = PRIORS[form]
    seen = set()
    for R in (1, 4, 5, 9):                                          # four rows per workgroup and its edge
        for counts in ([[n] for n in range(T + 1)] if R == 1 else [None]):
            a = logweight_inputs(T, R, A, seed=10 * R + A, counts=counts)
            seen |= set(a["n"].tolist())
            got = run_logweight_bwd(a, A, pr)
            ref = IT.reference_logweight_grad(*[a[k] for k in NAMES], a["presence"], a["g"], pr)
            for name, g, r in zip(NAMES + ("rec", "logp"), got, ref):
                assert np.isfinite(g).all(), (name, R)                # nothing left unwritten, rows of steps t >= n included
                assert same_bits(g, r), (name, R, A, form, np.abs(g - r).max())
            for g in got[:6]:
                assert not g[a["presence"] < 0.5].any()
    assert seen == set(range(T + 1))


@pytest.mark.parametrize("A", [50, 5])
def test_a_zero_scale_does_not_disturb_the_other_rows(gpu_device, A):
    R = 9
    a = logweight_inputs(T, R, A, seed=77, counts=[3] * R)
    clean = run_logweight_bwd(a, A, PRIORS["centred"])
    a["what_scale"][1, 5, A - 1] = 0.0
    a["where_scale"][2, 6, 1] = 0.0
    hit = run_logweight_bwd(a, A, PRIORS["centred"])
    ref = IT.reference_logweight_grad(*[a[k] for k in NAMES], a["presence"], a["g"], PRIORS["centred"])
    for name, c, h, r in zip(NAMES + ("rec", "logp"), clean, hit, ref):
        assert same_bits(h, r), name
        keep = np.ones(c.shape, bool)
        if name.startswith("what"):
            keep[1, 5, A - 1] = False
        elif name.startswith("where"):
            keep[2, 6, 1] = False
        assert same_bits(c[keep], h[keep]), name
    assert not np.isfinite(hit[2][1, 5, A - 1]) and not np.isfinite(hit[5][2, 6, 1])


# ---- air_iw_vimco --------------------------------------------------------------------------------------------------------------------
def run_vimco(lw, K):
    from attend_infer_repeat_amd import hip as H
    out = H.iw_vimco(torch.from_numpy(np.ascontiguousarray(lw, np.float32)).reshape(-1).cuda(), K)
    torch.cuda.synchronize()
    return dict(zip(("bound", "wnorm", "signal", "ess", "degenerate"), (o.cpu().numpy() for o in out)))


def check_vimco(got, ref, K, tag):
    bound = np.repeat(ref["bound"], K)
    for name in ("bound", "wnorm", "signal", "ess"):
        r = ref[name]
        scale = bound if r.shape[0] == bound.shape[0] else ref["bound"]
        tol = np.maximum(np.spacing(np.abs(r).astype(np.float32)).astype(np.float64), 2.0 ** -40 * np.maximum(1.0, np.abs(scale)))
        err = np.abs(got[name].astype(np.float64) - r)
        print("vimco %s %s: worst error / bar = %.3f" % (tag, name, (err / tol).max()))
        assert (err <= tol).all(), (tag, name, (err / tol).max())
    assert np.array_equal(got["degenerate"], ref["degenerate"])


@pytest.mark.parametrize("K", [2, 3, 5, 64, 65, 130])
def test_vimco_matches_the_float64_restatement(gpu_device, K):
    from test_iw_eval import run_reduce
    rng = np.random.default_rng(K)
    for B in (1, 4, 5):
        lw = rng.uniform(-730.0, -670.0, (B, K)).astype(np.float32)      # a naive exp underflows
        got = run_vimco(lw, K)
        ref = IT.reference_vimco(lw.reshape(-1), K)
        check_vimco(got, ref, K, "K=%d B=%d" % (K, B))
        assert np.abs(got["wnorm"].reshape(B, K).astype(np.float64).sum(1) - 1.0).max() <= K * 2.0 ** -24
        # the evaluation read-out's bound on the same log-weights: its float32 sum of K terms <= 1 and the rounding of its shift
        red = run_reduce(torch.from_numpy(lw).cuda(), torch.zeros((B, K), dtype=torch.int32, device="cuda"), T)["iw_bound"].cpu().numpy()
        bar = 4 * np.spacing(np.abs(got["bound"])).astype(np.float64) + K * 2.0 ** -23
        assert (np.abs(red.astype(np.float64) - got["bound"].astype(np.float64)) <= bar).all(), (K, B)


@pytest.mark.parametrize("K", [2, 5, 65])
def test_vimco_degenerate_images_are_zeroed_and_leave_their_neighbours_alone(gpu_device, K):
    rng = np.random.default_rng(100 + K)
    B = 6
    lw = rng.uniform(-730.0, -670.0, (B, K)).astype(np.float32)
    clean = run_vimco(lw, K)
    lw[1, K - 1] = np.nan
    lw[3, 0] = np.inf
    lw[4, :] = -np.inf
    got = run_vimco(lw, K)
    ref = IT.reference_vimco(lw.reshape(-1), K)
    assert got["degenerate"].tolist() == [0, 1, 0, 1, 1, 0]
    check_vimco(got, ref, K, "planted K=%d" % K)
    for b in (1, 3, 4):
        assert got["bound"][b] == 0.0 and got["ess"][b] == 0.0
        assert not got["wnorm"].reshape(B, K)[b].any() and not got["signal"].reshape(B, K)[b].any()
    for b in (0, 2, 5):
        for name in ("bound", "ess"):
            assert same_bits(got[name][b], clean[name][b])
        for name in ("wnorm", "signal"):
            assert same_bits(got[name].reshape(B, K)[b], clean[name].reshape(B, K)[b])
    if K > 2:                                                      # a single -inf is a weight of 0, not a degenerate image
        lw = rng.uniform(-730.0, -670.0, (2, K)).astype(np.float32)
        lw[0, 1] = -np.inf
        got = run_vimco(lw, K)
        assert got["degenerate"].tolist() == [0, 0] and got["wnorm"][1] == 0.0 and np.isfinite(got["signal"]).all()
        check_vimco(got, IT.reference_vimco(lw.reshape(-1), K), K, "one -inf K=%d" % K)


# ---- the tiny golden model -----------------------------------------------------------------------------------------------------------
B_TINY, K_TINY = 3, 4
TINY = O.tiny_config(step_bias=0.3, explore_eps=1e-3, output_multiplier=0.5, output_std=0.3, transform_var_bias=0.5)


def tiny_model(with_baseline=False, **step_kw):
    """AIRModel on the first B_TINY images of tests/golden/model_tiny.npz with its parameters; returns (model, train_step, baseline)"""
    import attend_infer_repeat_amd as amd
    from attend_infer_repeat_amd import cell, model, modules, neural, rnn, utils  # noqa: F401
    from test_api import _build_model, _load_oracle_params
    d = np.load(os.path.join(G, "model_tiny.npz"))
    params = {k[6:]: torch.tensor(d[k]) for k in d.files if k.startswith("param/")}
    obs = torch.tensor(d["obs"][:B_TINY]).cuda()
    m = _build_model(amd, TINY, obs, "lstm")
    AD = amd.utils.AttrDict
    nsp = AD(anneal='exp', init=TINY.nsp_init, final=TINY.nsp_final, steps_div=TINY.nsp_steps_div, steps=TINY.nsp_steps,
             hold_init=TINY.nsp_hold_init)
    baseline = amd.modules.BaselineMLP(list(TINY.baseline_hidden)) if with_baseline else None
    prior = AD(loc=0., scale=1.)
    ts, _ = m.train_step(TINY.learning_rate, 0., prior, AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp, baseline=baseline, **step_kw)
    _load_oracle_params(amd, m.cell, m.baseline_module if with_baseline and m.baseline_module is not None else None, params, "lstm")
    return m, ts, baseline, params


def tiny_noise(rows, seed=31):
    return {k: v.cuda() for k, v in O.make_noise(TINY, rows, seed=seed).items()}


def test_autograd_pair_against_a_float64_restatement(gpu_device):
    from attend_infer_repeat_amd import functional as F
    K, R = K_TINY, B_TINY * K_TINY
    m, _, _, _ = tiny_model(iw_samples=K)
    with torch.no_grad():
        m.obs, m.batch_size = m.obs.repeat_interleave(K, 0), R
        m.forward(noise=tiny_noise(R))
        rec = F.rec_loglik(m.obs, m._canvas_unscaled[-1], float(m.output_multiplier), m.output_std)
        prior = O.geometric_prior(0.3, T).cuda().double()
        presence = m.presence.reshape(T, R).contiguous()
        logq = F.numsteps(m.presence_prob.reshape(T, R).contiguous(), presence, prior)[2]
    n = presence.sum(0).long()
    assert len(set(n.tolist())) > 1, n
    pr = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    vals = [getattr(m, k).detach().clone() for k in NAMES] + [rec.clone(), logq.clone()]
    leaves = [v.requires_grad_(True) for v in vals]
    logw, n_dev = F.iw_logweight(*leaves[:6], presence, leaves[6], leaves[7], prior, K, pr)
    assert torch.equal(n_dev.long(), n)
    bound, sur = F.vimco(logw, leaves[7], K)
    got = torch.autograd.grad(sur, leaves)

    # the same objective in torch float64 on the same values: wnorm and signal are constants of the backward
    l64 = [v.detach().double().requires_grad_(True) for v in vals]
    what, what_loc, what_scale, where, where_loc, where_scale, rec64, logq64 = l64
    N = torch.distributions.Normal
    one = torch.ones((), dtype=torch.float64, device="cuda")
    live = (torch.arange(T, device="cuda")[:, None] < n[None, :]).double()
    ratio = (N(0 * one, one).log_prob(what) - N(what_loc, what_scale).log_prob(what)).sum(-1) \
        + (N(0 * one, one).log_prob(where) - N(where_loc, where_scale).log_prob(where)).sum(-1)
    logw64 = -rec64 + torch.log(prior)[n] - logq64 + (live * ratio).sum(0)
    assert ((logw.detach().double() - logw64.detach()).abs() <= 2.0 ** -18 * logw64.detach().abs().max()).all()
    # (the coefficients from the very log-weights the device folded: they are constants, the same values on both sides)
    ref = IT.reference_vimco(logw.detach().cpu().numpy(), K)
    assert not ref["degenerate"].any()
    wn, sg = (torch.from_numpy(ref[k]).cuda() for k in ("wnorm", "signal"))
    sur64 = -((wn * logw64).sum() + (sg * logq64).sum()) / B_TINY
    want = torch.autograd.grad(sur64, l64)
    assert abs(float(sur.detach()) + ref["bound"].mean()) <= 2.0 ** -18 * abs(ref["bound"].mean())
    for name, g, w in zip(NAMES + ("rec", "logq"), got, want):
        err = ((g.double() - w).abs().max() / w.abs().max()).item()
        print("autograd %s: worst / max = %.3e" % (name, err))
        assert err <= 2.0 ** -18, (name, err)
    # without the learning signal (use_reinforce=False) logq keeps only its share of log w
    leaves2 = [v.detach().clone().requires_grad_(True) for v in vals]
    sur2 = F.vimco(F.iw_logweight(*leaves2[:6], presence, leaves2[6], leaves2[7], prior, K, pr)[0], None, K)[1]
    g2 = torch.autograd.grad(sur2, leaves2)
    assert torch.equal(g2[7], g2[6]) and not torch.equal(g2[7], got[7])       # (d log w / d rec = d log w / d logq = -1)
    for a, b in zip(g2[:7], got[:7]):
        assert torch.equal(a, b)


def reduce_bar(bound, K):
    b = np.abs(np.asarray(bound, np.float32))
    return 4 * np.spacing(b).astype(np.float64) + K * 2.0 ** -23


def test_one_update_end_to_end_on_the_tiny_model(gpu_device):
    from test_iw_eval import engine_config
    from attend_infer_repeat_amd.iw_eval import ImportanceEvaluator
    K, R = K_TINY, B_TINY * K_TINY
    m, ts, baseline, params = tiny_model(with_baseline=True, iw_samples=K)
    noise = tiny_noise(R)
    before = [p.detach().clone() for p in m.cell.parameters()]
    assert int(ts(noise=noise)) == 1
    after = list(m.cell.parameters())
    assert all(torch.isfinite(p).all() for p in after)
    for p in after:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    # (centred RMSProp from its initial slots moves a parameter by about lr * g: a gradient that small against its parameter may
    # round away, so what is asked for is a move wherever the gradient is large enough to show in float32)
    for p, b in zip(after, before):
        big = (p.grad.abs() > 1e-2 * (b.abs() + 1e-3))
        assert (p[big] != b[big]).all()
    named = {"steps": m.cell._steps_predictor.mlp.layers[1].b, "decoder": m.cell._glimpse_decoder.mlp.layers[1].b,
             "what": m.cell._what_distrib.b}
    for k, p in named.items():
        assert any(p is q and not torch.equal(q, b) for q, b in zip(after, before)), k
    # no baseline: nothing was built, nothing is stepped
    assert m.baseline_module is None and m.baseline_vars == [] and float(m.baseline_loss) == 0.0
    assert all(l.w is None for l in baseline.mlp.layers)
    # the attributes: the caller's batch stays, the rows are K * B
    assert m.batch_size == B_TINY and tuple(m.obs.shape) == (B_TINY, 3, 3)
    assert tuple(m.what.shape) == (T, R, TINY.n_appearance) and tuple(m.rec_loss_per_sample.shape) == (R,)
    assert tuple(m.iw_bound_per_sample.shape) == (B_TINY,) and tuple(m.loss.per_sample.shape) == (R,)
    assert int(m.iw_degenerate) == 0 and 1.0 - 1e-5 <= float(m.iw_ess) <= K + 1e-4
    assert abs(float(m.iw_bound) - m.iw_bound_per_sample.double().mean().item()) <= 1e-5 * abs(float(m.iw_bound))
    assert float(m.opt_loss.detach()) == -float(m.iw_bound)
    assert float(m.iw_bound) >= -float(m.loss.value) - 1e-5 * abs(float(m.loss.value))          # the bound is above the ELBO of its rows
    # the evaluator's bound on the same parameters, images and noise (the un-normalised table of the training loss, step 0)
    ev = ImportanceEvaluator(engine_config(TINY), B_TINY, K, normalize_steps_prior=False)
    ev.load_parameters(params)
    ev.engine.set_noise(noise["eps_where"], noise["eps_what"], noise["u_pres"])
    ev.set_global_step(0)
    out = ev.evaluate(m.obs, sample_noise=False)
    ev.synchronize()
    assert torch.equal(out["num_steps"].reshape(-1).long(), m.presence.reshape(T, R).sum(0).long())
    got, ref = m.iw_bound_per_sample.cpu().numpy(), out["iw_bound"].cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("iw_bound: train", got.tolist(), "evaluator", ref.tolist(), "error / bar", (err / reduce_bar(ref, K)).tolist())
    assert (err <= reduce_bar(ref, K)).all()


def test_without_the_learning_signal_and_with_l2(gpu_device):
    K, R = K_TINY, B_TINY * K_TINY
    noise = tiny_noise(R)
    m1, ts1, _, _ = tiny_model(iw_samples=K)
    m2, ts2, _, _ = tiny_model(iw_samples=K, use_reinforce=False)
    ts1(noise=noise); ts2(noise=noise)
    assert torch.equal(m1.iw_bound_per_sample, m2.iw_bound_per_sample)
    steps = lambda m: m.cell._steps_predictor.mlp.layers[1].w.grad
    dec = lambda m: m.cell._glimpse_decoder.mlp.layers[1].w.grad
    assert torch.equal(dec(m1), dec(m2)) and not torch.equal(steps(m1), steps(m2))


def test_iw_samples_none_is_the_step_of_today(gpu_device):
    noise = tiny_noise(B_TINY, seed=32)
    a, ts_a, _, _ = tiny_model(with_baseline=True)
    b, ts_b, _, _ = tiny_model(with_baseline=True, iw_samples=None)
    ts_a(noise=noise); ts_b(noise=noise)
    for p, q in zip(list(a.cell.parameters()) + list(a.baseline_module.parameters()),
                    list(b.cell.parameters()) + list(b.baseline_module.parameters())):
        assert torch.equal(p, q)
    assert torch.equal(a.opt_loss, b.opt_loss) and torch.equal(a.baseline_loss, b.baseline_loss)
    assert not hasattr(b, "iw_bound") and b._iw_samples is None


def test_refusals(gpu_device):
    for kw, word in ((dict(iw_samples=1), "default objective"), (dict(iw_samples=4, decay_rate=0.9), "decay_rate"),
                     (dict(iw_samples=4, use_prior=False), "use_prior")):
        with pytest.raises(ValueError, match=word):
            tiny_model(**kw)


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def test_aironmnist_passes_iw_samples_through(gpu_device):
    from attend_infer_repeat_amd import mnist_model, utils
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    AD = utils.AttrDict
    B, K = 4, 2
    imgs, nums = synthetic_multi_mnist(B, (50, 50), 2, seed=0)
    x, y = torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda()
    torch.manual_seed(0)
    air = mnist_model.AIRonMNIST(x, y, max_steps=3, explore_eps=1e-3, steps_pred_hidden=[128, 64], transform_var_bias=.5,
                                 step_bias=.75, output_multiplier=.5, iw_samples=K)
    nsp = AD(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    ts, gs = air.train_step(1e-4, 0., AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp)
    assert air._engine is None and air._iw_samples == K                       # the generic path: no engine, no plans, no graphs
    assert air.baseline_module is None
    for _ in range(2):
        ts(x, y)
    assert int(gs) == 2 and torch.isfinite(air.iw_bound) and int(air.iw_degenerate) == 0
    assert tuple(air.what.shape) == (3, B * K, 50) and 0.0 <= float(air.num_step_accuracy) <= 1.0
    assert all(torch.isfinite(p).all() for p in air.cell.parameters())
    air.evaluate(x, y)                                                        # the logger's pass: the default objective on B rows
    assert tuple(air.what.shape) == (3, B, 50) and torch.isfinite(air.loss.value)
    with pytest.raises(ValueError, match="default objective"):
        air.train_step(1e-4, 0., AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.), nsp, iw_samples=1)


def test_training_script_iw_train_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "2", "--log-every", "2", "--save-every", "2", "--synthetic-samples", "256", "--eval-batches", "1",
                            "--summary-every", "1", "--results-dir", str(tmp_path), "--iw-train", "2"])
    capsys.readouterr()
    assert air._engine is None and int(air.global_step) == 2
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    summ = [l for l in lines if l["data"] == "summary"]
    assert [l["step"] for l in summ] == [1, 2]
    for l in summ:
        assert l["iw_samples"] == 2 and np.isfinite(l["iw_bound"]) and 1.0 - 1e-5 <= l["iw_ess"] <= 2.0 + 1e-4
        assert l["iw_degenerate"] == 0 and l["iw_degenerate_total"] == 0
    assert os.path.exists(os.path.join(tmp_path, "multi_mnist", "model_2.pt"))
