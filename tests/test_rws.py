"""GPU tests of training by reweighted wake-sleep (csrc/iw_train_kernels.hip: air_iw_logposterior_bwd; functional.iw_logposterior;
AIRCell.detach_samples; AIRModel.train_step(iw_samples=K, iw_objective="rws")): the entry against its host restatement
(iw_train.reference_logposterior_grad), the autograd function against a float64 restatement in torch, one update end to end on the
tiny golden model next to the VIMCO objective, the theta / phi split, the default, a degenerate image and the public surface.

Bars.  air_iw_logposterior_bwd is element-wise float32 without contraction: bit for bit against the restatement.  The autograd
gradients are a coefficient within one float32 ulp times an element-wise derivative within a few: 2^-18 of each tensor's largest
element (the bar of test_iw_train.py's pair test)."""
import json
import os

import numpy as np
import pytest
import torch

from attend_infer_repeat_amd import iw_train as IT
from oracle import air_oracle as O
from test_iw_train import B_TINY, K_TINY, T, TINY, same_bits, tiny_model, tiny_noise
from test_iw_train_host import NAMES, logweight_inputs

pytestmark = pytest.mark.gpu

OUT_NAMES = NAMES + ("logp",)


# ---- air_iw_logposterior_bwd ---------------------------------------------------------------------------------------------------------
def run_logposterior_bwd(a, A, K, samples=True):
    """the entry through the C ABI on output buffers filled with NaN: an element the kernel does not write shows"""
    from attend_infer_repeat_amd import _lib, hip as H
    steps, R = a["what"].shape[:2]
    dev = {k: torch.from_numpy(np.ascontiguousarray(a[k])).cuda() for k in NAMES + ("presence", "g")}
    outs = [torch.full(s, float("nan"), device="cuda") for s in [(steps, R, A)] * 3 + [(steps, R, 4)] * 3 + [(R,)]]
    ptrs = [H._p(o) for o in outs]
    if not samples:
        ptrs[0] = ptrs[3] = None
    st = H.lib().air_iw_logposterior_bwd(*[H._p(dev[k]) for k in NAMES + ("presence", "g")], steps, R, K, A, *ptrs, H._stream())
    _lib.check(st, "air_iw_logposterior_bwd")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def check_against_restatement(a, A, K, tag):
    ref = IT.reference_logposterior_grad(*[a[k] for k in NAMES], a["presence"], a["g"])
    dead = a["presence"] < 0.5
    for samples in (True, False):
        got = run_logposterior_bwd(a, A, K, samples)
        for name, g, r in zip(OUT_NAMES, got, ref):
            if not samples and name in ("what", "where"):
                assert np.isnan(g).all(), (name, tag)                # a NULL output: nothing was written anywhere near it
                continue
            assert np.isfinite(g).all(), (name, tag)                 # nothing left unwritten, rows of steps t >= n included
            assert same_bits(g, r), (name, tag, samples, np.abs(g - r).max())
            if name != "logp":
                assert not g[dead].any(), (name, tag)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("A", [50, 6, 5, 8])                       # V = 2, 2, 1, 4
def test_logposterior_bwd_is_the_host_restatement_bit_for_bit(gpu_device, A, K):
    R = 4 * K                                                       # B = 4: two and three workgroups of four rows
    a = logweight_inputs(T, R, A, seed=10 * K + A)
    assert set(a["n"].tolist()) == set(range(T + 1))
    check_against_restatement(a, A, K, "A=%d K=%d" % (A, K))


def test_logposterior_bwd_at_the_step_limit(gpu_device):
    """T = 32, R = 5, A = 5: a row tail inside the second workgroup, T * A = 160 items for 64 lanes (three strides, the last one
    partial), every lane below T on the `where` rows.  R = 5 rows hold five counts at a time: seven launches cover 0..32."""
    steps, R, A = 32, 5, 5
    order = np.random.default_rng(0).permutation(steps + 1)
    seen = set()
    for i in range(0, steps + 1, R):
        counts = np.resize(order[i:i + R], R)
        a = logweight_inputs(steps, R, A, seed=200 + i, counts=counts)
        seen |= set(a["n"].tolist())
        check_against_restatement(a, A, R, "T=32 counts=%s" % counts.tolist())
    assert seen == set(range(steps + 1))


@pytest.mark.parametrize("A", [50, 5])
def test_a_zero_scale_does_not_disturb_the_other_rows(gpu_device, A):
    R, K = 9, 3
    a = logweight_inputs(T, R, A, seed=77, counts=[3] * R)
    clean = run_logposterior_bwd(a, A, K)
    a["what_scale"][1, 5, A - 1] = 0.0
    a["where_scale"][2, 6, 1] = 0.0
    hit = run_logposterior_bwd(a, A, K)
    ref = IT.reference_logposterior_grad(*[a[k] for k in NAMES], a["presence"], a["g"])
    for name, c, h, r in zip(OUT_NAMES, clean, hit, ref):
        assert same_bits(h, r), name
        keep = np.ones(c.shape, bool)
        if name.startswith("what"):
            keep[1, 5, A - 1] = False
        elif name.startswith("where"):
            keep[2, 6, 1] = False
        assert same_bits(c[keep], h[keep]), name
    assert not np.isfinite(hit[2][1, 5, A - 1]) and not np.isfinite(hit[5][2, 6, 1])


# ---- the tiny golden model -----------------------------------------------------------------------------------------------------------
def tiled_forward(m, K, noise, grad=False):
    """the K-tiled unroll of a tiny model the way _iw_forward_losses runs it; returns rec [R], presence [T, R], logq [R], prior"""
    from attend_infer_repeat_amd import functional as F
    R = B_TINY * K
    if m.batch_size != R:
        m.obs, m.batch_size = m.obs.repeat_interleave(K, 0), R
    with torch.enable_grad() if grad else torch.no_grad():
        m.forward(noise=noise)
        rec = F.rec_loglik(m.obs, m._canvas_unscaled[-1], float(m.output_multiplier), m.output_std)
        prior = O.geometric_prior(0.3, T).cuda().double()
        presence = m.presence.reshape(T, R).contiguous()
        logq = F.numsteps(m.presence_prob.reshape(T, R).contiguous(), presence, prior)[2]
    return rec, presence, logq, prior


def test_autograd_against_a_float64_restatement(gpu_device):
    from attend_infer_repeat_amd import functional as F
    K, R = K_TINY, B_TINY * K_TINY
    m, _, _, _ = tiny_model(iw_samples=K, iw_objective="rws")
    rec, presence, logq, prior = tiled_forward(m, K, tiny_noise(R))
    n = presence.sum(0).long()
    assert len(set(n.tolist())) > 1, n
    vals = [getattr(m, k).detach().clone() for k in NAMES] + [rec.clone(), logq.clone()]
    with torch.no_grad():
        logw = F.iw_logweight(*vals[:6], presence, vals[6], vals[7], prior, K, (0.0, 1.0, 0.0, 1.0, 0.0, 1.0))[0]
    ref = IT.reference_vimco(logw.cpu().numpy(), K)                  # the coefficients from the device's own log-weights
    assert not ref["degenerate"].any()
    wn = torch.from_numpy(ref["wnorm"]).cuda()

    leaves = [v.requires_grad_(True) for v in vals]
    log_q = F.iw_logposterior(*leaves[:6], presence, leaves[7], K)
    sur = (wn.float() * (leaves[6] - log_q)).sum() / B_TINY
    got = torch.autograd.grad(sur, leaves)

    l64 = [v.detach().double().requires_grad_(True) for v in vals]
    what, what_loc, what_scale, where, where_loc, where_scale, rec64, logq64 = l64
    N = torch.distributions.Normal
    live = (torch.arange(T, device="cuda")[:, None] < n[None, :]).double()
    log_q64 = logq64 + (live * (N(what_loc, what_scale).log_prob(what).sum(-1) + N(where_loc, where_scale).log_prob(where).sum(-1))).sum(0)
    err = ((log_q.detach().double() - log_q64.detach()).abs().max() / log_q64.detach().abs().max()).item()
    print("forward log_q: worst / max = %.3e" % err)
    assert err <= 2.0 ** -18
    want = torch.autograd.grad((wn * (rec64 - log_q64)).sum() / B_TINY, l64)
    for name, g, w in zip(NAMES + ("rec", "logq"), got, want):
        err = ((g.double() - w).abs().max() / w.abs().max()).item()
        print("autograd %s: worst / max = %.3e" % (name, err))
        assert err <= 2.0 ** -18, (name, err)
    # fixed samples: their gradients are not asked for, the others are the same bits
    fixed = [v.detach().clone().requires_grad_(k not in (0, 3)) for k, v in enumerate(vals)]
    log_q2 = F.iw_logposterior(*fixed[:6], presence, fixed[7], K)
    assert torch.equal(log_q2, log_q)
    g2 = torch.autograd.grad((wn.float() * (fixed[6] - log_q2)).sum() / B_TINY, [fixed[k] for k in (1, 2, 4, 5, 6, 7)])
    for a, b in zip(g2, [got[k] for k in (1, 2, 4, 5, 6, 7)]):
        assert torch.equal(a, b)


def test_one_update_end_to_end_next_to_the_vimco_objective(gpu_device):
    K, R = K_TINY, B_TINY * K_TINY
    m, ts, baseline, _ = tiny_model(with_baseline=True, iw_samples=K, iw_objective="rws")
    v, ts_v, _, _ = tiny_model(iw_samples=K)
    assert m.iw_objective == "rws" and v.iw_objective == "vimco"
    before = [p.detach().clone() for p in m.cell.parameters()]
    assert int(ts(noise=tiny_noise(R))) == 1 and int(ts_v(noise=tiny_noise(R))) == 1
    after = list(m.cell.parameters())
    assert all(torch.isfinite(p).all() for p in after)
    for p in after:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    named = {"steps": m.cell._steps_predictor.mlp.layers[1].b, "decoder": m.cell._glimpse_decoder.mlp.layers[1].b,
             "what": m.cell._what_distrib.b}
    for k, p in named.items():
        assert any(p is q and not torch.equal(q, b) for q, b in zip(after, before)), k
    # no baseline: nothing was built, nothing is stepped; the flag is back where it was
    assert m.baseline_module is None and m.baseline_vars == [] and float(m.baseline_loss) == 0.0
    assert all(l.w is None for l in baseline.mlp.layers)
    assert m.cell.detach_samples is False
    assert m.batch_size == B_TINY and tuple(m.what.shape) == (T, R, TINY.n_appearance)
    # what describes the bound is formed as on the VIMCO path: the same bits on the same parameters and noise
    for name in ("iw_bound_per_sample", "iw_ess", "iw_log_weights", "num_step_per_sample", "iw_bound", "iw_degenerate"):
        assert torch.equal(getattr(m, name), getattr(v, name)), name
    assert torch.equal(m.loss.value, v.loss.value) and torch.equal(m.loss.per_sample, v.loss.per_sample)
    assert torch.isfinite(m.opt_loss) and float(m.opt_loss.detach()) != -float(m.iw_bound)      # a surrogate, not the bound
    # the decoder follows sum wnorm grad(-rec) under both objectives; the inference side does not
    dec = {id(p) for p in m.cell._glimpse_decoder.parameters()}
    assert dec
    differs = 0
    for p, q in zip(m.cell.parameters(), v.cell.parameters()):
        if id(p) in dec:
            err = ((p.grad.double() - q.grad.double()).abs().max() / q.grad.double().abs().max()).item()
            print("decoder gradient %s: worst / max = %.3e, bit-equal: %s" % (tuple(p.shape), err, torch.equal(p.grad, q.grad)))
            assert err <= 2.0 ** -18
        else:
            differs += int(not torch.equal(p.grad, q.grad))
    assert differs >= 1


def test_the_split_holds(gpu_device):
    from attend_infer_repeat_amd import functional as F
    K, R = K_TINY, B_TINY * K_TINY
    m, _, _, _ = tiny_model(iw_samples=K, iw_objective="rws")
    params = list(m.cell.parameters())
    dec = {id(p) for p in m.cell._glimpse_decoder.parameters()}
    coef = torch.rand(R, generator=torch.Generator().manual_seed(3)).cuda() + 0.1
    names = list(m.cell.output_names) + ["final_canvas"]

    def pass_(flag):
        m.cell.detach_samples = flag
        try:
            rec, presence, logq, _ = tiled_forward(m, K, tiny_noise(R), grad=True)
        finally:
            m.cell.detach_samples = False
        log_q = F.iw_logposterior(m.what, m.what_loc, m.what_scale, m.where, m.where_loc, m.where_scale, presence, logq, K)
        outs = [getattr(m, k).detach().clone() for k in names] + [rec.detach().clone(), log_q.detach().clone()]
        g_rec = torch.autograd.grad((coef * rec).sum(), params, allow_unused=True, retain_graph=True)
        g_q = torch.autograd.grad((coef * log_q).sum(), params, allow_unused=True)
        return outs, g_rec, g_q

    zero = lambda g: g is None or not g.any()
    outs_set, g_rec, g_q = pass_(True)
    for p, gr, gq in zip(params, g_rec, g_q):
        if id(p) in dec:
            assert zero(gq) and not zero(gr), tuple(p.shape)        # the decoder: grad log p(x, z) only
        else:
            assert zero(gr), tuple(p.shape)                          # everything else: grad log q only
    assert sum(int(not zero(gq)) for p, gq in zip(params, g_q) if id(p) not in dec) >= 4
    outs_clear, g_rec_clear, _ = pass_(False)
    for name, a, b in zip(names + ["rec", "log_q"], outs_set, outs_clear):
        assert torch.equal(a, b), name                               # the forward does not see the flag
    # with the flag clear the reconstruction term does reach the inference network through the samples: the flag is what cuts it
    assert any(not zero(g) for p, g in zip(params, g_rec_clear) if id(p) not in dec)


def test_off_by_default(gpu_device):
    K, R = K_TINY, B_TINY * K_TINY
    models = [tiny_model(iw_samples=K, **kw) for kw in ({}, dict(iw_objective=None), dict(iw_objective="vimco"))]
    for m, ts, _, _ in models:
        ts(noise=tiny_noise(R))
        assert m.iw_objective == "vimco" and m.cell.detach_samples is False
    for m, _, _, _ in models[1:]:
        for p, q in zip(models[0][0].cell.parameters(), m.cell.parameters()):
            assert torch.equal(p, q)
        assert torch.equal(models[0][0].opt_loss, m.opt_loss)
    plain, _, _, _ = tiny_model()
    assert plain.iw_objective is None
    for kw, word in ((dict(iw_objective="rws"), "needs iw_samples"), (dict(iw_samples=K, iw_objective="iwae"), "iw_objective must be"),
                     (dict(iw_samples=K, iw_objective="rws", use_reinforce=False), "use_reinforce=False")):
        with pytest.raises(ValueError, match=word):
            tiny_model(**kw)


def test_a_degenerate_image_takes_no_part(gpu_device, monkeypatch):
    from attend_infer_repeat_amd import model as M
    K, R = K_TINY, B_TINY * K_TINY
    m, ts, _, _ = tiny_model(iw_samples=K, iw_objective="rws")
    real = M.F.rec_loglik

    def planted(*args, **kw):                                         # a NaN in rec of image 1, particle 2, before the surrogate is formed
        rec = real(*args, **kw)
        bad = torch.zeros_like(rec)
        bad[1 * K + 2] = float("nan")
        return rec + bad

    monkeypatch.setattr(M.F, "rec_loglik", planted)
    ts(noise=tiny_noise(R))
    assert int(m.iw_degenerate) == 1 and torch.isnan(m.rec_loss_per_sample).sum() == 1
    coef = m.iw_weights.reshape(B_TINY, K)
    assert not coef[1].any()                                          # zero coefficients on its K rows ...
    for b in (0, 2):                                                  # ... and the others share the mean over two images
        assert abs(float(coef[b].sum()) - 0.5) <= 1e-6
    assert torch.isfinite(m.opt_loss) and torch.isfinite(m.iw_bound)
    for p in m.cell.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and torch.isfinite(p).all()
    assert m.cell._glimpse_decoder.mlp.layers[1].b.grad.any()


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def test_aironmnist_passes_iw_objective_through(gpu_device):
    from attend_infer_repeat_amd import mnist_model, utils
    from attend_infer_repeat_amd.data import synthetic_multi_mnist
    AD = utils.AttrDict
    B, K = 4, 2
    imgs, nums = synthetic_multi_mnist(B, (50, 50), 2, seed=0)
    x, y = torch.from_numpy(imgs).cuda(), torch.from_numpy(nums).cuda()
    torch.manual_seed(0)
    air = mnist_model.AIRonMNIST(x, y, max_steps=3, explore_eps=1e-3, steps_pred_hidden=[128, 64], transform_var_bias=.5,
                                 step_bias=.75, output_multiplier=.5, iw_samples=K, iw_objective="rws")
    nsp = AD(anneal='exp', init=1. - 1e-15, final=1e-7, steps_div=1e4, steps=1e5, hold_init=1e3)
    priors = (AD(loc=0., scale=1.), AD(loc=0., scale=1.), AD(loc=0., scale=1.))
    ts, gs = air.train_step(1e-4, 0., *priors, nsp)
    assert air._engine is None and air._iw_samples == K and air.iw_objective == "rws"        # the generic path
    assert air.baseline_module is None
    for _ in range(2):
        ts(x, y)
    assert int(gs) == 2 and torch.isfinite(air.iw_bound) and int(air.iw_degenerate) == 0
    assert tuple(air.what.shape) == (3, B * K, 50) and not air.what.requires_grad and air.what_loc.requires_grad
    assert all(torch.isfinite(p).all() for p in air.cell.parameters())
    _, _ = air.train_step(1e-4, 0., *priors, nsp, iw_objective="vimco")                       # the argument wins over the constructor's
    assert air.iw_objective == "vimco"


def test_training_script_iw_objective_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "2", "--log-every", "2", "--save-every", "2", "--synthetic-samples", "256", "--eval-batches", "1",
                            "--summary-every", "1", "--results-dir", str(tmp_path), "--iw-train", "2", "--iw-objective", "rws"])
    capsys.readouterr()
    assert air._engine is None and int(air.global_step) == 2 and air.iw_objective == "rws"
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    summ = [l for l in lines if l["data"] == "summary"]
    assert [l["step"] for l in summ] == [1, 2]
    for l in summ:
        assert l["iw_samples"] == 2 and l["iw_objective"] == "rws" and np.isfinite(l["iw_bound"]) and np.isfinite(l["opt_loss"])
