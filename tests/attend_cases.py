"""Case builders and float64 references for the kernel-level tests of the fused launches around the glimpse read (air_attend_fwd,
air_attend_bwd, air_attend_bwd_dx) and of the `what` head (air_what_head_fwd, air_what_sample_pack), plus the helpers the
kernel-level test modules share (tests/test_objective_kernels.py, tests/test_attend_kernels.py).  Importable without a GPU;
tests/test_attend_cases_host.py builds every case on the CPU and checks the references against independent ones.  No test lives here.

References are written out with torch in float64 on the functions of oracle/air_oracle.py and oracle/st_loops.py.  Inputs are built so
that no comparison has to leave an element out; every such condition is asserted where the input is made:
  * every |u - p64| >= U_MARGIN, so that no presence draw can flip between float32 and float64 (the GPU test asserts that the kernel's
    p stays within a tenth of that);
  * continuous steps: sum_t p at least 0.05 away from an integer (the count is its floor);
  * no tr_y / st_y entry within 1e-3 of 0, the kink of elu';
  * `where` rows inside the ranges of rand_where, so that every glimpse overlaps its image;
  * every reference is finite."""
import functools

import numpy as np
import torch

from oracle import air_oracle as O
from oracle import st_loops as C

WORST = {}                  # group letter -> (worst error / tolerance ratio, what), filled by assert_close


def g(x, dtype=torch.float32):
    if x is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def assert_close(a, b, rtol, atol, what="", group=None):
    """err <= atol + rtol * |b| for every element (the semantics of tests/test_hip_kernels.py), shapes equal"""
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} against {b.shape}"
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    if group is not None and err.size:
        ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
        worst = float(np.nanmax(ratio)) if np.isfinite(ratio).any() else float("inf")
        if group not in WORST or worst > WORST[group][0]:
            WORST[group] = (worst, what)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e} (tol {tol.flat[err.argmax()]:.3e}) at {np.unravel_index(err.argmax(), err.shape)}"


def assert_bits(a, b, what=""):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    same = a.view(torch.int32) == b.view(torch.int32) if a.dtype == torch.float32 else a == b
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in their bits"


def print_worst(title, groups):
    for grp in sorted(WORST):
        if grp in groups:
            ratio, what = WORST[grp]
            print(f"\n[{title}] group {grp}: worst error / tolerance = {ratio:.3g} ({what})")


def rand_where(B, rng, wide=False):
    sx = rng.uniform(0.2, 1.4, B) * (rng.choice([-1, 1], B) if wide else 1)
    sy = rng.uniform(0.2, 1.4, B)
    return np.stack([sx, rng.uniform(-0.8, 0.8, B), sy, rng.uniform(-0.8, 0.8, B)], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the count side (shared with tests/test_objective_kernels.py)
# ---------------------------------------------------------------------------------------------------------------
NSP = 0.3                                                                       # success probability of the geometric prior


def _rev_cumsum(q):
    """step weights w[t, b] = sum_{n > t} q[b, n] from q[B, T+1]"""
    return torch.flip(torch.cumsum(torch.flip(q[:, 1:].t(), [0]), 0), [0])


def _posterior_refs(prob32, count, prior):
    """the oracle path of test_numsteps_fwd_bwd: the f32 posterior, re-cast to f64 inside tabular_kl like the reference"""
    q = O.bernoulli_to_modified_geometric(prob32.t())
    return q, O.tabular_kl(q, prior[None]).sum(1), _rev_cumsum(q), O.num_steps_log_prob(q, count)


def _objective64(p64, count, prior, kl_scale, dw, dlogp):
    """kl_scale * KL + sum(w * dw) + sum(dlogp * logp) in float64 (terms given as None are left out)"""
    q64 = O.bernoulli_to_modified_geometric(p64.t())
    L = kl_scale * O.tabular_kl(q64, prior[None]).sum()
    if dw is not None:
        L = L + (_rev_cumsum(q64) * dw.double()).sum()
    if dlogp is not None:
        L = L + (O.num_steps_log_prob(q64, count) * dlogp.double()).sum()
    return L


def _presence_prob64(l64, step_bias, eps):
    p = torch.sigmoid(l64 + step_bias)
    return p if eps is None else eps / 2 + (1 - eps) * p


def _margin_u(u, p64, margin=1e-5):
    """u with every element at least `margin` away from the float64 p (the kernel's p is within 1e-6 p + 1e-7 of it), so that
    (u < p) is the same in the kernel and in float64 and the Bernoulli chain can be compared exactly"""
    u64 = u.double()
    near = (u64 - p64).abs() < margin
    u = torch.where(near, torch.where(u64 >= p64, p64 + 2 * margin, p64 - 2 * margin), u64).float()
    assert bool(((u.double() - p64).abs() >= margin).all())
    return u


def _check_fused_forward(out, c, prior, tag, group="A"):
    """prob against the float64 chain; presence exactly; q / KL / w / log q(n*) against the oracle's f32-posterior path evaluated on
    the prob the kernel wrote.  (The posterior is ill-conditioned in p near 1: q(n) carries (1 - p_n), so one float32 ulp of p at
    p = 1 - 1e-4 moves q(n) by 6e-8, six times its atol.  Feeding the oracle the written prob keeps the tolerances of the generic
    kernel's test meaningful, and still fails if the posterior was formed from any other p than the one written.)"""
    prob, pres, q, kl, logp, w = out
    assert_close(prob, c["p64"], 1e-6, 1e-7, tag + "prob", group)
    if c["u"] is None:
        assert_bits(pres, prob, tag + "presence = prob")
    else:
        assert torch.equal(pres.cpu().double(), c["pres"]), tag + "presence"
    rq, rkl, rw, rlogp = _posterior_refs(prob.cpu(), c["count"], prior)
    assert_close(q, rq, 1e-6, 1e-8, tag + "q", group); assert_close(kl, rkl, 1e-5, 1e-6, tag + "kl", group)
    assert_close(w, rw, 1e-6, 1e-7, tag + "w", group); assert_close(logp, rlogp, 1e-5, 1e-6, tag + "logp", group)


# name, continuous, kl_a, kl_b, dlogp, dpresence, step_bias, explore_eps
BWD_VARIANTS = [
    ("discrete, both kl rows, dlogp", False, True, True, True, False, 0.75, 1e-3),
    ("discrete, kl_b only, no dlogp, no eps", False, False, True, False, False, 0.0, None),
    ("discrete, kl_a only, dlogp", False, True, False, True, False, 0.0, 1e-3),
    ("discrete, no kl rows, dlogp, no eps", False, False, False, True, False, 0.75, None),
    ("continuous, both kl rows, dlogp, dpresence", True, True, True, True, True, 0.75, 1e-3),
    ("continuous, dpresence alone, no eps", True, False, False, False, True, 0.0, None),
    ("continuous, both kl rows, dlogp, no dpresence", True, True, True, True, False, 0.0, None),
]
KL_SCALE, W_SCALE = 0.37, 1.0 / 64


# ---------------------------------------------------------------------------------------------------------------
# the attend launches: inputs and the float64 forward
# ---------------------------------------------------------------------------------------------------------------
RAW_OFFSET = 0.5
PRIOR4 = (0.3, 1.5, -0.2, 0.7)              # prior loc / scale of the even (scale) and of the odd (shift) dimensions of `where`
DKL_SCALE = 0.7
U_MARGIN = 1e-4
_EVEN = torch.tensor([True, False, True, False])


def _rounded(precision):
    return O._r16 if precision else (lambda t: t)


def where_head64(pre, eps, guard_eps=0.0):
    """pre[M, 8], eps[M, 4] in float64 -> loc (sigmoid on the even dimensions, tanh on the odd ones), scale = softplus(raw + offset),
    where = loc + scale * eps, the KL row against the two priors"""
    loc = torch.where(_EVEN, torch.sigmoid(pre[:, :4]), torch.tanh(pre[:, :4]))
    scale = O._guard_scale(O.softplus(pre[:, 4:] + RAW_OFFSET), guard_eps)
    where = loc + scale * eps
    if guard_eps > 0:                                                           # |where scale| >= guard_eps, straight through
        sgn = torch.where(torch.signbit(where), -torch.ones_like(where), torch.ones_like(where))
        where = where + (torch.where(_EVEN & (where.abs() < guard_eps), sgn * guard_eps, where) - where).detach()
    pl = torch.tensor([PRIOR4[0], PRIOR4[2]] * 2, dtype=torch.float64); ps = torch.tensor([PRIOR4[1], PRIOR4[3]] * 2, dtype=torch.float64)
    return dict(loc=loc, scale=scale, where=where, kl_row=O.normal_kl(loc, scale, pl, ps).sum(-1))


def products64(c):
    """pre = tr_h . tr_w + tr_b and logit = st_h . st_w + st_b in float64 on the float32 operands (rounded to bf16 first for precision 1)"""
    r = _rounded(c["precision"])
    pre = r(c["tr_h"]).double() @ r(c["tr_w"]).double() + c["tr_b"].double()
    logit = r(c["st_h"]).double() @ r(c["st_w"]).double() + c["st_b"].double()
    return pre, logit.reshape(c["T"], c["B"])


def attend_inputs(seed, T, B, H, W, h, w, tr_k, st_k, precision, continuous, step_bias, explore_eps, guard_eps=0.0):
    """float32 inputs of one air_attend_fwd launch with its float64 reference outputs (everything but q / KL / w / log q(n*), which
    _check_fused_forward forms from the prob the kernel wrote)"""
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    M = T * B
    c = dict(T=T, B=B, H=H, W=W, h=h, w=w, tr_k=tr_k, st_k=st_k, precision=precision, step_bias=step_bias, explore_eps=explore_eps,
             guard_eps=guard_eps, continuous=continuous)
    c["img"] = torch.as_tensor((rng.random((B, H, W)) * (rng.random((B, H, W)) < 0.5)).astype(np.float32))
    c["tr_h"] = torch.randn(M, tr_k, generator=gen); c["tr_w"] = torch.randn(tr_k, 8, generator=gen) * 0.7 / tr_k ** 0.5
    c["tr_b"] = torch.randn(8, generator=gen) * 0.3
    c["st_h"] = torch.randn(M, st_k, generator=gen); c["st_w"] = torch.randn(st_k, generator=gen) * 2 / st_k ** 0.5
    c["st_b"] = torch.randn(1, generator=gen) * 0.3
    if guard_eps > 0:
        # row 0: push the raw scale of dimension 0 to about -12 along its own weight column, so that softplus lands below the floor
        v = c["tr_w"][:, 4].double()
        pre0 = products64(c)[0][0, 4]
        c["tr_h"][0] += ((-12.0 - pre0) / (v * v).sum() * v).float()
    if continuous:
        # the count is int(sum_t p): keep the sum at least 0.05 away from an integer, so that the order of a float32 sum cannot move it
        for _ in range(200):
            frac = torch.remainder(_presence_prob64(products64(c)[1], step_bias, explore_eps).sum(0), 1.0)
            bad = (frac < 0.05) | (frac > 0.95)
            if not bool(bad.any()):
                break
            c["st_h"].view(T, B, st_k)[:, bad] = torch.randn(T, int(bad.sum()), st_k, generator=gen)
    pre, logit = products64(c)
    p64 = _presence_prob64(logit, step_bias, explore_eps)
    if continuous:
        frac = torch.remainder(p64.sum(0), 1.0)
        assert bool(((frac >= 0.05) & (frac <= 0.95)).all())
        c.update(u=None, pres=p64, count=torch.floor(p64.sum(0)))
    else:
        c["u"] = _margin_u(torch.rand(T, B, generator=gen), p64, U_MARGIN)
        assert bool(((c["u"].double() - p64).abs() >= U_MARGIN).all())
        c["pres"] = torch.cumprod((c["u"].double() < p64).double(), 0)
        c["count"] = c["pres"].sum(0)
    # eps such that `where` lands on a row of rand_where: every glimpse overlaps its image
    target = torch.as_tensor(rand_where(M, rng)).double()
    head = where_head64(pre, torch.zeros(M, 4, dtype=torch.float64), guard_eps)
    c["eps"] = ((target - head["loc"]) / head["scale"]).float()
    ref = where_head64(pre, c["eps"].double(), guard_eps)
    wh = ref["where"]
    assert bool(((wh[:, 0::2] >= 0.2 - 1e-4) & (wh[:, 0::2] <= 1.4 + 1e-4) & (wh[:, 1::2].abs() <= 0.8 + 1e-4)).all())
    if guard_eps > 0:
        assert float(O.softplus(pre[0, 4] + RAW_OFFSET)) < guard_eps and float(ref["scale"][0, 0]) == guard_eps
        assert int((ref["scale"] <= guard_eps).sum()) == 1
    c.update(pre64=pre, logit64=logit, p64=p64, prior=O.geometric_prior(NSP, T), **{k + "64": v for k, v in ref.items()})
    for k in ("pre64", "logit64", "p64", "loc64", "scale64", "where64", "kl_row64", "eps"):
        assert bool(torch.isfinite(c[k]).all()), k
    return c


F32, BF16 = 0, 1
# T, B, H, W, h, w, tr_k, st_k, precision, u given, step_bias, explore_eps, guard_eps
# (air_attend_fwd picks 256 / 512 / 1024 threads by nq = H*W/4, <3> / <5> / <8> / <32> by T, image-major beyond 2048 glimpses)
FWD_CASES = [
    (3, 5, 50, 50, 20, 20, 256, 50, F32, True, 0.75, 1e-3, 0.0),        # nq = 625: 256 threads; exact <3>; one glimpse per workgroup
    (5, 70, 100, 100, 28, 28, 200, 33, F32, True, 0.0, None, 0.0),      # nq = 2500, T*B = 350 > 256: 512 threads; exact <5>; tr_k, st_k no multiple of 64 / 4; two role-B workgroups
    (5, 4, 100, 100, 28, 28, 64, 1, BF16, True, 0.75, 1e-3, 0.0),       # T*B = 20: 1024 threads; bf16 operands; st_k = 1 (three of the four lanes of a column idle)
    (7, 3, 28, 36, 9, 12, 40, 7, F32, False, 0.0, None, 0.0),           # T = 7: <8> generic; u == NULL; tr_k < 64 (lanes without a k)
    (8, 9, 28, 36, 9, 12, 40, 7, F32, False, 0.75, 1e-3, 0.0),          # T = 8: the edge of <8>; u == NULL with the eps mix
    (9, 9, 28, 36, 9, 12, 300, 50, F32, True, 0.75, 1e-3, 0.0),         # T = 9: the first <32>
    (32, 3, 12, 10, 3, 4, 20, 20, BF16, True, 0.0, 1e-3, 0.0),          # T = 32: the last <32>; bf16; tr_k = st_k = 20
    (32, 65, 12, 10, 3, 4, 64, 16, F32, True, 0.75, 1e-3, 0.0),         # 2080 glimpses: image-major, lean (w % 4 == 0), T = 32 above the 4 waves (t += nwv wraps, wf0 = 0: all waves busy); st_k = 16: 16-byte role-B loads
    (9, 230, 17, 12, 5, 7, 40, 7, F32, True, 0.0, None, 0.0),           # 2070 glimpses: image-major, w % 4 != 0: the per-pixel form, where rows in c.scratch, T above the wave count
    (6, 342, 28, 36, 9, 12, 72, 48, F32, True, 0.75, None, 0.0),        # 2052 glimpses: image-major, lean, generic <8>
    (2, 1030, 12, 10, 3, 4, 20, 33, F32, False, 0.0, 1e-3, 0.0),        # 2060 glimpses: image-major, lean, T = 2 below the wave count (wf0 = 2: waves 2, 3 fill the tables); u == NULL; 17 role-B workgroups
    (2, 1030, 8, 1, 3, 4, 20, 7, F32, True, 0.0, None, 0.0),            # image-major, w % 4 == 0 but W = 1: a 16-byte group of the image spans four rows, which the lean staging cannot place: the per-pixel form
    (3, 5, 50, 50, 20, 20, 256, 50, F32, True, 0.75, 1e-3, 1e-3),       # the guard: one scale floored at guard_eps = 1e-3
]
FWD_UNSUPPORTED = (3, 2, 7, 5, 3, 4, 40, 7)                             # H*W % 4 != 0: AIR_E_UNSUPPORTED before any launch


@functools.lru_cache(maxsize=None)
def fwd_case(i):
    T, B, H, W, h, w, tr_k, st_k, precision, has_u, step_bias, explore_eps, guard_eps = FWD_CASES[i]
    return attend_inputs(4000 + i, T, B, H, W, h, w, tr_k, st_k, precision, not has_u, step_bias, explore_eps, guard_eps)


# ---------------------------------------------------------------------------------------------------------------
# the attend backward
# ---------------------------------------------------------------------------------------------------------------
# T, B, H, W, h, w, (tr_k, tr_ld), (st_k, st_ld), tr_y given, st_y given, slabs, row of BWD_VARIANTS, dkl_row given, precision of the _dx run
# (attend_bwd_launch picks the threads by h*w: <= 256, <= 512, beyond; image-major beyond 2048 glimpses: 256 threads up to h*w = 1024;
#  its fast form while T * (nw * 8 + 8) <= 3 w + 3 h + 160.  Role B of the _dx form: 16 columns per workgroup, nout = 16 * T * st_k.)
BWD_CASES = [
    (3, 5, 50, 50, 20, 20, (256, 260), (50, 53), True, True, 2, 0, True, F32),      # h*w = 400: 512 threads; exact <3>; tr_ld > tr_k, st_ld > st_k; B < 16: one ragged role-B workgroup
    (5, 4, 100, 100, 28, 28, (40, 40), (130, 130), False, True, 1, 4, True, F32),   # h*w = 784: 1024 threads; exact <5>; tr_y NULL; nout = 10400 > 4 * 1024: the second role-B pass; continuous with dpresence
    (7, 19, 28, 36, 9, 12, (600, 604), (50, 53), True, True, 3, 1, True, F32),      # h*w = 108: 256 threads; <8>; B % 16 != 0, two role-B workgroups; tr_k = 600 > 2 * 256: the strided loop and its tr_y load at tr_ld; kl_row_a, dlogp NULL
    (9, 17, 28, 36, 9, 12, (256, 260), (130, 130), True, False, 4, 5, True, BF16),  # <32>; st_y NULL; four slabs; bf16 dX; kl_row_a, kl_row_b, dlogp NULL, dpresence alone
    (2, 6, 7, 5, 3, 4, (40, 40), (1, 1), True, True, 1, 3, False, F32),             # H*W = 35: vec4 = 0 (scalar staging); dkl_row NULL; st_k = 1; kl rows NULL
    (4, 520, 12, 10, 3, 4, (40, 40), (50, 53), True, True, 2, 2, True, F32),        # 2080 glimpses, 160 <= 181: image-major fast form, generic <8>; kl_row_b NULL; without st_dx ceil(520 / 64) = 9 role-B workgroups
    (3, 704, 50, 50, 20, 20, (256, 260), (1, 1), True, False, 3, 6, True, F32),     # 2112 glimpses, 120 <= 280: image-major fast form, exact <3>, h*w = 400 on 256 threads; dpresence NULL on the continuous path
    (5, 417, 12, 10, 3, 4, (600, 604), (130, 130), True, True, 4, 0, True, BF16),   # 2085 glimpses, 200 > 181: image-major per-glimpse loop (c.scratch reused from glimpse to glimpse), exact <5>; tr_k > 2 nt there; bf16 dX
    (32, 65, 12, 10, 3, 4, (256, 260), (50, 53), True, True, 2, 4, True, F32),      # 2080 glimpses: image-major per-glimpse loop, <32>
    (2, 1030, 50, 50, 36, 36, (40, 40), (50, 53), False, False, 1, 0, True, F32),   # 2060 glimpses, h*w = 1296 > 1024: image-major on 1024 threads, 16 waves: 272 <= 376, the fast form; tr_y and st_y NULL
]
SENTINEL = 12345.0                                                      # fills the padding columns of tr_dx / st_dx


def elu_prime(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def _elu_output(gen, rows, cols):
    """an ELU output (> -1) with no entry within 1e-3 of 0, the kink of elu'"""
    y = torch.nn.functional.elu(torch.randn(rows, cols, generator=gen))
    y = torch.where(y.abs() < 1e-3, torch.full_like(y, 2e-3), y)
    assert bool((y.abs() >= 1e-3).all()) and bool((y > -1).all())
    return y


def dpre_ref(c, dwhere_r):
    """float64 autograd of sum(where(pre) * (sum_slabs dwhere_w + dwhere_r)) + dkl_scale * sum(dkl_row * kl_row(pre)) at the float32 pre
    handed to the kernel"""
    pre = c["pre"].double().requires_grad_(True)
    head = where_head64(pre, c["eps"].double())
    ds = c["dwhere_w"].double().sum(0) + torch.as_tensor(dwhere_r).double()
    L = (head["where"] * ds).sum()
    if c["dkl_row"] is not None:
        L = L + DKL_SCALE * (c["dkl_row"].double() * head["kl_row"]).sum()
    gp, = torch.autograd.grad(L, [pre])
    return gp


def dx_ref(c, dpre, dlogit, precision):
    """tr_dx = (dpre . tr_w^T) * elu'(tr_y), st_dx = dlogit (x) st_w * elu'(st_y); operands rounded to bf16 for precision 1"""
    r = _rounded(precision)
    tr = r(dpre.float().cpu()).double() @ r(c["tr_w"]).double().t()
    st = r(dlogit.float().cpu()).double().reshape(-1, 1) * r(c["st_w"]).double()[None, :]
    if c["tr_y"] is not None:
        tr = tr * elu_prime(c["tr_y"].double())
    if c["st_y"] is not None:
        st = st * elu_prime(c["st_y"].double())
    return tr, st


@functools.lru_cache(maxsize=None)
def bwd_case(i):
    T, B, H, W, h, w, (tr_k, tr_ld), (st_k, st_ld), has_try, has_sty, slabs, variant, has_dkl, precision = BWD_CASES[i]
    name, continuous, has_a, has_b, has_dlogp, has_dpres, step_bias, explore_eps = BWD_VARIANTS[variant]
    # the forward reference, rounded to float32: what the kernel is handed (never the output of the forward kernel under test)
    f = attend_inputs(7000 + i, T, B, H, W, h, w, 16, 8, F32, continuous, step_bias, explore_eps)
    gen = torch.Generator().manual_seed(7100 + i)
    M = T * B
    c = dict(T=T, B=B, H=H, W=W, h=h, w=w, tr_k=tr_k, tr_ld=tr_ld, st_k=st_k, st_ld=st_ld, slabs=slabs, precision=precision, name=name,
             continuous=continuous, step_bias=step_bias, explore_eps=explore_eps, img=f["img"], eps=f["eps"], prior=f["prior"], u=f["u"],
             p64=f["p64"], count=f["count"])
    for k in ("where", "loc", "scale", "pre", "logit"):
        c[k] = f[k + "64"].float()
    c["prob"] = f["p64"].float()
    c["presence"] = c["prob"] if continuous else f["pres"].float()
    c["dglimpse"] = torch.randn(M, h, w, generator=gen) * 0.1
    c["dwhere_w"] = torch.randn(slabs, M, 4, generator=gen)
    c["dkl_row"] = torch.randn(M, generator=gen) if has_dkl else None
    c["ka"] = torch.rand(T, B, generator=gen) * 4 if has_a else None
    c["kb"] = torch.rand(T, B, generator=gen) * 40 if has_b else None
    c["dlogp"] = torch.randn(B, generator=gen) if has_dlogp else None
    c["dpres"] = torch.randn(T, B, generator=gen) if has_dpres else None
    c["tr_w"] = torch.randn(tr_k, 8, generator=gen) / 8 ** 0.5; c["st_w"] = torch.randn(st_k, generator=gen)
    c["tr_y"] = _elu_output(gen, M, tr_k) if has_try else None
    c["st_y"] = _elu_output(gen, M, st_k) if has_sty else None
    # d where through the read: the scalar loops of oracle/st_loops.c in float64, at the float32 `where`
    img64 = np.tile(c["img"].double().numpy(), (T, 1, 1))
    c["dwhere_r64"] = torch.as_tensor(C.st_read_bwd(img64, c["where"].double().numpy(), c["dglimpse"].double().numpy(), want_dimg=False)[0])
    # d logit: the objective of tests/test_objective_kernels.py (_bwd_case), plus dpresence on the continuous path
    l64 = c["logit"].double().requires_grad_(True)
    p = _presence_prob64(l64, step_bias, explore_eps)
    dw = None
    if has_a or has_b:
        dw = W_SCALE * ((c["ka"].double() if has_a else 0.0) + (c["kb"].double() if has_b else 0.0))
    L = _objective64(p, c["count"], c["prior"], KL_SCALE, dw, c["dlogp"])
    if has_dpres:
        L = L + (c["dpres"].double() * p).sum()
    c["dlogit64"], = torch.autograd.grad(L, [l64])
    c["dpre64"] = dpre_ref(c, c["dwhere_r64"])
    for k in ("dwhere_r64", "dlogit64", "dpre64"):
        assert bool(torch.isfinite(c[k]).all()), k
    return c


# ---------------------------------------------------------------------------------------------------------------
# the `what` head
# ---------------------------------------------------------------------------------------------------------------
WHAT_OFFSET, WHAT_PRIOR = 0.5, (0.1, 1.3)
# T, B, K, ldx, A, S0, S1, precision, x offset by one float
# (a tile is 16 rows x 8 latent dimensions; the pack role runs min(256, ceil(B * (5 T + S0 + S1) / 256)) workgroups)
WHAT_CASES = [
    (3, 5, 21, 21, 50, 256, 256, F32, True),        # x offset by one float: unaligned, the scalar loads; A % 8 = 2, M = 15 < 16, K % 4 != 0
    (5, 7, 64, 68, 12, 40, 0, F32, False),          # ldx > K on the 16-byte path; M = 35 = 2 tiles + 3 rows; S1 = 0
    (1, 1, 9, 12, 3, 0, 0, BF16, False),            # one row, one tile, no state parts; bf16 operands; A < 8
    (3, 130, 256, 256, 50, 256, 256, F32, False),   # B * (5 T + S0 + S1) = 68510 > 65536: the pack role's 256-workgroup cap, its loop wraps
    (2, 33, 30, 32, 8, 7, 5, F32, False),           # A = 8: exactly one tile column; M = 66 = 4 tiles + 2 rows; odd state widths
]


@functools.lru_cache(maxsize=None)
def what_case(i):
    T, B, K, ldx, A, S0, S1, precision, offset = WHAT_CASES[i]
    gen = torch.Generator().manual_seed(9000 + i)
    M = T * B
    c = dict(T=T, B=B, K=K, ldx=ldx, A=A, S0=S0, S1=S1, precision=precision, offset=offset)
    c["x_buf"] = torch.randn(M, ldx, generator=gen)                     # x = x_buf[:, :K]
    c["w"] = torch.randn(K, 2 * A, generator=gen) / K ** 0.5; c["b"] = torch.randn(2 * A, generator=gen) * 0.3
    c["eps"] = torch.randn(M, A, generator=gen)
    c["where"] = torch.randn(T, B, 4, generator=gen); c["presence"] = torch.rand(T, B, generator=gen)
    c["states"] = [torch.randn(B, s, generator=gen) for s in (S0, S1) if s > 0]
    assert S0 > 0 or S1 == 0
    r = _rounded(precision)
    q = r(c["x_buf"][:, :K]).double() @ r(c["w"]).double() + c["b"].double()
    c["q64"] = q; c["loc64"] = q[:, :A]
    c["scale64"] = O.softplus(q[:, A:] + WHAT_OFFSET)
    c["sample64"] = c["loc64"] + c["scale64"] * c["eps"].double()
    pl, ps = (torch.tensor(v, dtype=torch.float64) for v in WHAT_PRIOR)
    c["kl_row64"] = O.normal_kl(c["loc64"], c["scale64"], pl, ps).sum(-1)
    for k in ("q64", "scale64", "sample64", "kl_row64"):
        assert bool(torch.isfinite(c[k]).all()), k
    return c


def pack_ref(sample, where, presence, states, T, B):
    """pack_out[B, T*A + 4T + T + S0 + S1] = [what | where | presence | state0 | state1], batch-major, as an indexed copy"""
    A = sample.shape[1]
    cols = [t.permute(1, 0, 2).reshape(B, -1) for t in (sample.reshape(T, B, A), where, presence.reshape(T, B, 1))]
    return torch.cat(cols + list(states), -1)
