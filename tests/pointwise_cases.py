"""Case tables, builders, float64 references, float32 restatements, bounds and planted defects for the kernel-level tests of the
Gaussian nodes, the optimiser, the bf16 casts and the utilities (tests/test_pointwise_kernels.py): the rest of
csrc/pointwise_kernels.hip (gauss_fwd/bwd/bwd_nvil_kernel, normal_kl_fwd/bwd_kernel, rmsprop_kernel<true/false>,
step_epilogue_kernel<true/false>, f32_to_bf16_kernel / _vec_kernel, step_prologue_cvt_kernel, l2_grad_kernel, fill / axpby / tile_rows /
colsum) and the Gaussian half of the heads launches of csrc/engine_kernels.hip (heads_fwd/bwd_kernel<8> and <32>).  Importable without
a GPU; tests/test_pointwise_cases_host.py holds every reference against an independent one, the restatements' share of every bound,
the defects' margins and the coverage of the instantiations.  No test lives here.

Groups.
  Ga  air_gauss_sample_fwd / _bwd / _bwd_nvil, air_normal_kl_fwd / _bwd, air_heads_fwd / _bwd (Gaussian half): float64 autograd through
      oracle.air_oracle's normal_kl and softplus (sigmoid / tanh for loc_mode 1) at the float32 inputs the kernel is handed.
  Op  air_rmsprop (centred, plain), air_rmsprop_centered, air_step_epilogue / _shadow (vector and scalar form), the rider of
      air_lstm_pointwise_bwd_opt, air_l2_grad_add.  The centred update is held to the BITS of rmsprop32, a numpy float32 restatement of
      rmsprop_elem (csrc/optimizer_device.h) with one rounding per operation, NaN positions included.
  Bf  air_f32_to_bf16 (vector, scalar), the shadow of air_step_epilogue_shadow (both forms), the conversion workgroups of
      air_step_prologue_cvt: bits of an integer round-to-nearest-even; a NaN stays a NaN.
  Ut  air_fill, air_axpby, air_tile_rows, air_colsum.

Operands and outputs.  Every operand is a window of a NaN-filled parent, every output a NaN-primed window of a SENTINEL-filled parent
(Win / out_win of tests/warp_cases.py; Win16 here for bf16); in-place buffers of the optimiser are windows of SENTINEL parents.  The
test compares every parent for bits outside the window after the launch.

Bounds of Ga.  Elementwise |out - out64| <= CONST * 2^-24 * S with S from float64 quantities only: the sum of the magnitudes of the
summands of the element's analytic expression, the summands of raw = pre + offset carried through softplus / its derivative, and the
term through which ONE float32 rounding of the stored loc and scale (the operands of the backward) moves the result.  Each CONST is
four times the worst ratio of the numpy float32 restatement of the same formulas on the same inputs, rounded up (GA_RATIO below, printed
and held to RESTATEMENT_SHARE by the host test) -- never a GPU result.

What cannot be planted.  A `where` scale sample of -0: the sample is sigmoid(pre) + scale * eps and sigmoid is never -0, so +0 + (-0) =
+0 is the nearest reachable (the row with eps = -0 is kept: it must give +guard).  A sample EXACTLY at the guard: both branches of
guard_where give the guard there, and scale * eps cannot be hit to the bit through softplus; the row sits within a rounding of it.
A forward scale exactly at the guard: softplus cannot be hit to the bit either; the three scales at / under / over the guard are
planted in the STORED scale of the backward, where `s <= guard` decides."""
import functools

import numpy as np
import torch

import fold_cases as FC
from attend_cases import SENTINEL
from oracle import air_oracle as O
from warp_cases import DEFECT_MARGIN, NAN, RESTATEMENT_SHARE, U32, Win, out_win, surroundings_intact  # noqa: F401  (re-exported)

F32 = np.float32
CAP_ITEMS = 2048 * 256                      # pw_blocks / blocks_for: at most 2048 workgroups of 256 threads
CAP_ROWS = CAP_ITEMS // 64                  # one 64-lane wave per row
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -5         # AIR_E_* of include/air_hip.h
GUARD = 1e-3
PRIOR_A, PRIOR_B = (0.3, 1.5, -0.2, 0.7), (0.0, 1.0, NAN, 0.7)


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


class Win16:
    """Win for 16-bit elements: a window of a uint16 parent filled with `fill` (outputs: SENTINEL16 around a NaN-primed inside), 16
    (+1 when `off`: 2 bytes past an 8-byte boundary) elements in front, 16 behind"""
    SENTINEL16, PRIMER16 = 0x5A5A, 0x7FC1

    def __init__(self, n, off=False):
        self.n, self.lead = int(n), 16 + int(bool(off))
        self.parent = torch.full((self.lead + self.n + 16,), self.SENTINEL16, dtype=torch.int32).to(torch.int16)
        self.parent[self.lead:self.lead + self.n] = self.PRIMER16

    def cuda(self):
        p = self.parent.cuda()
        return p, p[self.lead:self.lead + self.n]

    def intact(self, dev_parent):
        p = dev_parent.cpu().to(torch.int32) & 0xFFFF
        return bool((torch.cat([p[:self.lead], p[self.lead + self.n:]]) == self.SENTINEL16).all())


def state_win(values, off=False):
    """an in-place buffer: `values` as the window of a SENTINEL parent"""
    v = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.float32)
    w = Win(v.shape, off, SENTINEL)
    w.v.copy_(v)
    return w


def same_bits_or_nan(a, b):
    """-> number of elements that differ: a NaN must meet a NaN (sign and payload not compared), anything else its bits"""
    a, b = np.ascontiguousarray(a, dtype=F32).ravel(), np.ascontiguousarray(b, dtype=F32).ravel()
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.int32) != b.view(np.int32)))).sum())


# ===============================================================================================================
# Ga. the Gaussian nodes
# ===============================================================================================================
def _parity(prior4, D, dtype=torch.float64):
    pl0, ps0, pl1, ps1 = prior4
    odd = torch.arange(D) % 2 == 1
    return (odd, torch.where(odd, torch.tensor(pl1, dtype=dtype), torch.tensor(pl0, dtype=dtype)),
            torch.where(odd, torch.tensor(ps1, dtype=dtype), torch.tensor(ps0, dtype=dtype)))


def gauss64(pre, eps, D, loc_mode, offset, prior4, guard=0.0, defect=None):
    """the head in float64 through the oracle's formulas: pre [M, >= 2D] (float64, may require grad), eps [M, D] | None ->
    loc, scale, sample | None, kl_row.  A NaN prior mean is the posterior's own mean (no mean term, no gradient through it).
    guard > 0: the scale floor and the straight-through floor of the sampled even components of a loc_mode 1 head.
    Defects: "parity" (the two priors swapped), "nan_kept" (a NaN prior mean taken as 0: the term kept)"""
    prior4 = tuple(FC.f32v(v) for v in prior4)
    if defect == "parity":
        prior4 = prior4[2:] + prior4[:2]
    odd, pm, ps = _parity(prior4, D)
    x = pre[:, :D]
    loc = torch.where(odd, torch.tanh(x), torch.sigmoid(x)) if loc_mode == 1 else x
    scale = O._guard_scale(O.softplus(pre[:, D:2 * D] + FC.f32v(offset)), FC.f32v(guard))
    own = torch.isnan(pm)
    if defect == "nan_kept":
        mean = torch.where(own, torch.zeros_like(pm), pm).expand_as(loc)
    else:
        mean = torch.where(own, loc, torch.where(own, torch.zeros_like(pm), pm).expand_as(loc))
    kl = O.normal_kl(loc, scale, mean, ps).sum(-1)
    sample = None
    if eps is not None:
        sample = loc + scale * eps
        if guard > 0 and loc_mode == 1:
            g_ = FC.f32v(guard)
            floor = torch.where(sample.detach() < 0, -g_, g_)
            hit = (~odd) & (sample.detach().abs() < g_)
            sample = torch.where(hit, sample + (floor - sample).detach(), sample)
    return loc, scale, sample, kl


def gauss_bwd64(pre, eps, D, loc_mode, offset, prior4, dsample, dsample2, dkl_row, dkl_scale, guard=0.0, defect=None):
    """float64 autograd of sum(sample * (dsample + dsample2)) + dkl_scale * sum(dkl_row * kl_row) at the float32 pre -> dpre [M, 2D].
    Defects: those of gauss64, "no_ds2" (dsample2 dropped), "no_dkl_scale" (dkl_scale taken as 1)"""
    p64 = torch.as_tensor(pre, dtype=torch.float64).clone().requires_grad_(True)
    e64 = None if eps is None else torch.as_tensor(eps, dtype=torch.float64)
    _, _, sample, kl = gauss64(p64, e64, D, loc_mode, offset, prior4, guard, defect)
    L = torch.zeros((), dtype=torch.float64)
    for ds in (dsample, None if defect == "no_ds2" else dsample2):
        if ds is not None:
            L = L + (sample * torch.as_tensor(ds, dtype=torch.float64)).sum()
    if dkl_row is not None:
        L = L + (1.0 if defect == "no_dkl_scale" else FC.f32v(dkl_scale)) * (torch.as_tensor(dkl_row, dtype=torch.float64) * kl).sum()
    L = L + 0.0 * p64.sum()
    gp, = torch.autograd.grad(L, [p64])
    return gp[:, :2 * D].numpy()


def _np_parity(prior4, D):
    odd = (np.arange(D) & 1).astype(bool)
    pl0, ps0, pl1, ps1 = (FC.f32v(v) for v in prior4)
    return odd, np.where(odd, pl1, pl0), np.where(odd, ps1, ps0)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def gauss_terms64(pre, eps, D, loc_mode, offset, prior4, loc=None, scale=None, dsample=None, dsample2=None, dkl_row=None,
                  dkl_scale=1.0, guard=0.0, defect=None):
    """the head written out by hand in float64 numpy: the values and S of every output.  loc / scale given: the STORED operands of the
    backward (else the float64 ones).  -> dict loc, scale, sample, kl_row, dpre and S_* of each (sample / dpre only when their inputs
    are given).  Defects (backward): "dsp_no_offset" (the derivative of softplus taken at raw without the offset), "tanh_even" (the tanh
    derivative on the even dimensions too)"""
    with np.errstate(all="ignore"):
        pre = np.asarray(pre, np.float64)
        off, g_ = FC.f32v(offset), FC.f32v(guard)
        odd, pm, ps = _np_parity(prior4, D)
        own = np.isnan(pm)
        x, rp = pre[:, :D], pre[:, D:2 * D]
        r = rp + off
        if loc_mode == 1:
            mu0 = np.where(odd, np.tanh(x), _sig(x))
            dmu_dx = np.where(odd, 1.0 - mu0 * mu0, mu0 * (1.0 - mu0))
        else:
            mu0, dmu_dx = x, np.ones_like(x)
        sg = np.where(r > 20.0, 1.0, _sig(r))
        s0 = np.where(r > 20.0, r, np.log1p(np.exp(r)))
        floored0 = (g_ > 0) & (s0 < g_)
        s0 = np.where(floored0, g_, s0)
        out = dict(loc=mu0, scale=s0)
        out["S_loc"] = np.abs(mu0) + np.abs(dmu_dx * x) if loc_mode == 1 else np.zeros_like(x)        # loc_mode 0: a copy, bits
        out["S_scale"] = np.where(floored0, 0.0, s0 + sg * (np.abs(rp) + abs(off)))
        d0 = np.where(own, 0.0, mu0 - np.where(own, 0.0, pm))
        ratio0 = s0 * s0 / (ps * ps)
        out["kl_row"] = (d0 * d0 / (2 * ps * ps) + 0.5 * (ratio0 - 1.0 - np.log(ratio0))).sum(1)
        out["S_kl_row"] = (d0 * d0 / (ps * ps) + np.abs(d0) / (ps * ps) * (np.abs(mu0) + np.where(own, 0.0, np.abs(pm)) + out["S_loc"])
                           + 0.5 * (ratio0 + 1.0 + np.abs(np.log(ratio0))) + np.abs(ratio0 - 1.0) * (1.0 + out["S_scale"] / s0)).sum(1)
        if eps is not None:
            e = np.asarray(eps, np.float64)
            v = mu0 + s0 * e
            if g_ > 0 and loc_mode == 1:
                v = np.where((~odd) & (np.abs(v) < g_), np.where(np.signbit(v), -g_, g_), v)
            out["sample"] = v
            out["S_sample"] = np.abs(mu0) + out["S_loc"] + (s0 + out["S_scale"]) * np.abs(e)
        if dkl_row is None and dsample is None and dsample2 is None:
            return out
        mu = mu0 if loc is None else np.asarray(loc, np.float64)
        s = s0 if scale is None else np.asarray(scale, np.float64)
        M = pre.shape[0]
        zero = np.zeros((M, D))
        ds1 = zero if dsample is None else np.asarray(dsample, np.float64)
        ds2 = zero if dsample2 is None else np.asarray(dsample2, np.float64)
        ds, ads = ds1 + ds2, np.abs(ds1) + np.abs(ds2)
        e = zero if eps is None else np.asarray(eps, np.float64)
        dk = zero[:, :1] if dkl_row is None else (np.asarray(dkl_row, np.float64) * FC.f32v(dkl_scale))[:, None]
        d = np.where(own, 0.0, mu - np.where(own, 0.0, pm))
        A = ds + dk * d / (ps * ps)
        S_A = ads + np.abs(dk) * np.where(own, 0.0, np.abs(mu) + np.abs(np.where(own, 0.0, pm))) / (ps * ps)
        if loc_mode == 1:
            tanh_like = np.ones(D, bool) if defect == "tanh_even" else odd
            f = np.where(tanh_like, 1.0 - mu * mu, mu * (1.0 - mu))
            fS = np.where(odd, 1.0 + mu * mu, np.abs(mu) * (1.0 + np.abs(mu)))
            df = np.where(odd, -2.0 * mu, 1.0 - 2.0 * mu)
            dloc = A * f
            S_dloc = S_A * np.abs(f) + np.abs(A) * (fS + np.abs(df * mu))
        else:
            dloc, S_dloc = A, S_A
        Bv = ds * e + dk * (s / (ps * ps) - 1.0 / s)
        S_B = ads * np.abs(e) + 2.0 * np.abs(dk) * (s / (ps * ps) + 1.0 / s)
        rr = rp if defect == "dsp_no_offset" else r
        dsp = np.where(rr > 20.0, 1.0, _sig(rr))
        floored = (g_ > 0) & (s <= g_)
        dsp = np.where(floored, 0.0, dsp)
        draw = Bv * dsp
        S_draw = S_B * dsp + np.abs(Bv) * dsp * (1.0 - dsp) * (np.abs(rp) + abs(off))
        out["dpre"] = np.concatenate([dloc, draw], 1)
        out["S_dpre"] = np.concatenate([S_dloc, S_draw], 1)
        return out


# ---- the float32 restatement (numpy, one rounding per operation, the kernel's order of operations) -------------------------------
def _fn32(fn, x):
    """a float32 library function: the float64 one rounded once (the same on every host, whatever its float32 libm)"""
    return fn(np.asarray(x, np.float64)).astype(F32)


def _sig32(x):
    return (F32(1) / (F32(1) + _fn32(np.exp, -x))).astype(F32)


def _softplus32(x):
    return np.where(x > F32(20), x, _fn32(np.log1p, _fn32(np.exp, x))).astype(F32)


def _kl_elem32(mu, s, pm, ps):
    own = np.isnan(pm)
    ratio = (s * s) / (ps * ps)
    d = np.where(own, F32(0), mu - np.where(own, F32(0), pm)).astype(F32)
    return (d * d / (F32(2) * ps * ps) + F32(0.5) * (ratio - F32(1) - _fn32(np.log, ratio))).astype(F32)


def wave_rows32(t):
    """t [M, D] float32 -> the row sums in the order of gauss_fwd_body / normal_kl_fwd_kernel: lane l adds its elements l, l + 64, ...
    in turn from 0.f, then wave_sum's tree (v[l] += v[l + off], off = 32 ... 1)"""
    M, D = t.shape
    k = -(-D // 64)
    pad = np.zeros((M, k * 64), F32)
    pad[:, :D] = t
    v = np.zeros((M, 64), F32)
    for j in range(k):
        v = (v + pad[:, j * 64:(j + 1) * 64]).astype(F32)
    off = 32
    while off:
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
        off >>= 1
    return v[:, 0].copy()


def gauss_fwd32(pre, eps, D, loc_mode, offset, prior4, guard=0.0):
    with np.errstate(all="ignore"):
        pre = np.asarray(pre, F32)
        odd, pm, ps = _np_parity(prior4, D)
        pm, ps, g_ = pm.astype(F32), ps.astype(F32), F32(guard)
        x = pre[:, :D]
        mu = np.where(odd, _fn32(np.tanh, x), _sig32(x)).astype(F32) if loc_mode == 1 else x.copy()
        s = _softplus32(pre[:, D:2 * D] + F32(offset))
        if g_ > 0:
            s = np.where(s < g_, g_, s).astype(F32)
        sample = None
        if eps is not None:
            sample = (mu + s * np.asarray(eps, F32)).astype(F32)
            if g_ > 0 and loc_mode == 1:
                sample = np.where((~odd) & (np.abs(sample) < g_), np.copysign(g_, sample), sample).astype(F32)
        return mu, s, sample, wave_rows32(_kl_elem32(mu, s, pm, ps))


def _dscale32(dk, s, ps):
    ps2 = ps * ps
    ratio = (s * s) / ps2
    gr = F32(0.5) * dk - (F32(0.5) * dk) / ratio
    return ((gr / ps2) * (F32(2) * s)).astype(F32)


def gauss_bwd32(pre, eps, D, loc_mode, offset, prior4, loc, scale, dsample, dsample2, dkl_row, dkl_scale, guard=0.0):
    """gauss_bwd_body / gauss_bwd_elem on the stored float32 loc and scale"""
    with np.errstate(all="ignore"):
        pre, mu, s = np.asarray(pre, F32), np.asarray(loc, F32), np.asarray(scale, F32)
        M = pre.shape[0]
        odd, pm, ps = _np_parity(prior4, D)
        pm, ps, g_ = pm.astype(F32), ps.astype(F32), F32(guard)
        zero = np.zeros((M, D), F32)
        ds = ((zero if dsample is None else np.asarray(dsample, F32)) + (zero if dsample2 is None else np.asarray(dsample2, F32))).astype(F32)
        has_ds = dsample is not None or dsample2 is not None
        e = np.asarray(eps, F32) if has_ds else zero
        dk = zero[:, :1] if dkl_row is None else (np.asarray(dkl_row, F32) * F32(dkl_scale))[:, None].astype(F32)
        own = np.isnan(pm)
        d = np.where(own, F32(0), mu - np.where(own, F32(0), pm)).astype(F32)
        dmu = (ds + dk * d / (ps * ps)).astype(F32)
        dsc = ((ds * e if has_ds else zero) + _dscale32(dk, s, ps)).astype(F32)
        if loc_mode == 1:
            dmu = (dmu * np.where(odd, F32(1) - mu * mu, mu * (F32(1) - mu))).astype(F32)
        raw = (pre[:, D:2 * D] + F32(offset)).astype(F32)
        dsp = np.where(raw > F32(20), F32(1), _sig32(raw)).astype(F32)
        if g_ > 0:
            dsp = np.where(s <= g_, F32(0), dsp).astype(F32)
        return np.concatenate([dmu, (dsc * dsp).astype(F32)], 1)


def normal_kl_bwd64(loc, scale, prior4, dkl):
    """air_normal_kl_bwd by hand on the float32 loc / scale it is handed -> dloc, dscale, S_dloc, S_dscale"""
    mu, s, g = np.asarray(loc, np.float64), np.asarray(scale, np.float64), np.asarray(dkl, np.float64)[:, None]
    odd, pm, ps = _np_parity(prior4, mu.shape[1])
    own = np.isnan(pm)
    pm0 = np.where(own, 0.0, pm)
    d = np.where(own, 0.0, mu - pm0)
    return (g * d / (ps * ps), g * (s / (ps * ps) - 1.0 / s), np.abs(g) * np.where(own, 0.0, np.abs(mu) + np.abs(pm0)) / (ps * ps),
            np.abs(g) * (s / (ps * ps) + 1.0 / s))


def normal_kl_bwd32(loc, scale, prior4, dkl):
    mu, s, g = np.asarray(loc, F32), np.asarray(scale, F32), np.asarray(dkl, F32)[:, None]
    odd, pm, ps = _np_parity(prior4, mu.shape[1])
    pm, ps = pm.astype(F32), ps.astype(F32)
    own = np.isnan(pm)
    d = np.where(own, F32(0), mu - np.where(own, F32(0), pm)).astype(F32)
    return (g * d / (ps * ps)).astype(F32), _dscale32(g, s, ps)


# one constant per kind of output: four times the worst ratio |restatement - float64| / (2^-24 S) over the cases, rounded up.  The
# worst ratios (tests/test_pointwise_cases_host.py prints them and asserts the share they leave): see GA_RATIO.
# loc: sigmoid as 1 / (1 + exp(-x)), three roundings (Ga_8197x4_where); dpre: d raw of Ga_41x50_no_kl [no_dkl]; kl_bwd: dscale of Ga_8197x65,
# the chain ratio = s s / ps^2, g/2 - (g/2) / ratio, / ps^2, * 2 s of normal_kl_dscale where scale is near the prior's
GA_RATIO = {"loc": 1.966, "scale": 1.231, "sample": 1.059, "kl_row": 0.537, "dpre": 2.602, "kl_bwd": 4.300}
GA_CONST = {"loc": 8.0, "scale": 5.0, "sample": 5.0, "kl_row": 3.0, "dpre": 11.0, "kl_bwd": 18.0}


FLT_MIN = 2.0 ** -126          # below the smallest normal float32 the format has no relative precision: sigmoid(-200) is 1.4e-87 in float64, 0 in float32


def ga_bound(kind, S):
    """CONST * 2^-24 * S, plus FLT_MIN wherever S > 0 (an element with S == 0 must be exact)"""
    S = np.asarray(S, np.float64)
    return GA_CONST[kind] * U32 * S + np.where(S > 0, FLT_MIN, 0.0)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# backward option rows: (dsample, dsample2, dkl_row, dkl_scale); eps is NULL exactly when there is no sample gradient
BWD_OPTS = {"ds_dkl": (1, 0, 1, 1.0), "ds_ds2": (1, 1, 1, 1.0), "ds2": (0, 1, 1, 1.0), "kl_only": (0, 0, 1, 1.0), "no_dkl": (1, 1, 0, 1.0),
            "scale07": (1, 0, 1, 0.7)}
GA = {}


def _ga(name, M, D, loc_mode, offset, prior4, fwd="full", bwd=("ds_dkl",), guard=0.0, plant=(), kl_bwd=False):
    """fwd: "full" | "no_sample" (sample and eps NULL) | "no_kl" (kl_row NULL); plant: names of planted_elements"""
    assert name not in GA
    GA[name] = dict(name=name, M=M, D=D, loc_mode=loc_mode, offset=offset, prior4=prior4, fwd=fwd, bwd=tuple(bwd), guard=guard,
                    plant=tuple(plant), kl_bwd=kl_bwd, ld_pre=2 * D + 3, ld_dpre=2 * D + 5)


_ga("Ga_1x1", 1, 1, 0, 0.5, PRIOR_A, kl_bwd=True)
_ga("Ga_3x4_where", 3, 4, 1, 0.5, PRIOR_A, bwd=("ds_dkl", "ds_ds2"))
_ga("Ga_41x50", 41, 50, 0, -2.0, PRIOR_A, bwd=tuple(BWD_OPTS), plant=("switch", "small"), kl_bwd=True)
_ga("Ga_41x50_nan_mean", 41, 50, 0, 0.5, PRIOR_B, bwd=("ds_dkl", "kl_only", "scale07"), plant=("switch", "small"), kl_bwd=True)
_ga("Ga_41x50_no_sample", 41, 50, 0, 0.5, PRIOR_A, fwd="no_sample", bwd=("kl_only",))
_ga("Ga_41x50_no_kl", 41, 50, 1, 0.5, PRIOR_A, fwd="no_kl", bwd=("no_dkl",))
_ga("Ga_5x64", 5, 64, 0, 0.5, PRIOR_A, kl_bwd=True)
_ga("Ga_5x65_where", 5, 65, 1, -2.0, PRIOR_B, bwd=("ds_dkl", "ds_ds2", "scale07"), plant=("switch", "saturated", "small"), kl_bwd=True)
_ga("Ga_7x200", 7, 200, 0, 0.5, PRIOR_A, bwd=("ds_dkl", "ds_ds2"), kl_bwd=True)
_ga("Ga_13x8_where_planted", 13, 8, 1, 0.5, PRIOR_A, bwd=("ds_dkl", "ds_ds2", "scale07"), plant=("switch", "saturated", "small"))
_ga("Ga_8197x4_where", CAP_ROWS + 5, 4, 1, 0.5, PRIOR_A, plant=("switch", "saturated"))              # the forward strides over rows
_ga("Ga_8197x65", CAP_ROWS + 5, 65, 0, -2.0, PRIOR_B, bwd=("ds_ds2", "scale07"), plant=("switch", "small"), kl_bwd=True)    # both stride
_ga("Ga_guard_where", 12, 4, 1, 0.5, PRIOR_A, bwd=("ds_dkl",), guard=GUARD, plant=("floored", "where_floor"))
_ga("Ga_guard_41x50", 41, 50, 0, 0.5, PRIOR_B, bwd=("ds_ds2",), guard=GUARD, plant=("floored", "small"))
GA_RUN = list(GA)
GA_STRIDED_FWD = ("Ga_8197x4_where", "Ga_8197x65")
GA_STRIDED_BWD = ("Ga_8197x65",)
# air_heads_fwd / _bwd against the stand-alone launches: (T, B), D = 4: M = T B above 8192 rows, so the Gaussian part of the grid sits
# at its cap in the forward (M * 64 items) and M * D = 32 896 items take 129 workgroups in the backward; T = 8 and 9: both templates
HEADS_TB = ((32, 257), (8, 1025), (9, 1025))
# refusals: entry, what is wrong, the status
GA_REFUSALS = (("fwd", "ld_pre", E_SHAPE), ("fwd", "loc_mode2", E_UNSUPPORTED), ("fwd", "M0", E_SHAPE), ("fwd", "sample_no_eps", E_NULL),
               ("bwd", "ld_pre", E_SHAPE), ("bwd", "ld_dpre", E_SHAPE), ("bwd", "M0", E_SHAPE), ("bwd", "ds_no_eps", E_NULL),
               ("bwd", "ds2_no_eps", E_NULL), ("bwd_nvil", "ds_no_eps", E_NULL), ("bwd_nvil", "M0", E_SHAPE),
               ("kl_fwd", "M0", E_SHAPE), ("kl_bwd", "null", E_NULL))
SWITCH_TARGETS = (float(np.nextafter(F32(20), F32(0))), 20.0, float(np.nextafter(F32(20), F32(40))), 30.0)


def _plant(c, pre, eps, rng):
    """-> {name: [(row, dim), ...]}; rows are taken from the front, one planted kind per row"""
    M, D, off = c["M"], c["D"], F32(c["offset"])
    at, row = {}, 0
    take = lambda: min(row, M - 1)
    if "switch" in c["plant"]:                      # raw + offset at the float32 below 20, 20, the float32 above 20, 30
        at["switch"] = []
        for i, t in enumerate(SWITCH_TARGETS):
            d = (3 * i + 1) % D
            pre[take(), D + d] = F32(t) - off
            assert float(F32(pre[take(), D + d] + off)) == t, (c["name"], t)
            at["switch"].append((take(), d))
        row += 1
    if "small" in c["plant"]:                       # raw + offset = -15: scale 3.06e-7, far above the underflow regime
        d = 2 % D
        pre[take(), D + d] = F32(-15.0) - off
        at["small"] = [(take(), d)]
        row += 1
    if "saturated" in c["plant"]:                   # loc_mode 1 pre-activations +-30: sigmoid and tanh saturated
        at["saturated"] = []
        for d, v in ((0, 30.0), (1 % D, 30.0), (2 % D, -30.0), (3 % D, -30.0)):
            pre[take(), d] = v
            at["saturated"].append((take(), d))
        row += 1
    if "floored" in c["plant"]:                     # softplus(raw + offset) = 6.1e-6 under the guard
        d = 1 % D
        pre[take(), D + d] = F32(-12.0) - off
        at["floored"] = [(take(), d)]
        row += 1
    if "where_floor" in c["plant"]:
        # the sampled scale components of a transform head (even dims): loc = sigmoid(-200) = +0 in float32 (1.4e-87 in float64), raw +
        # offset = 1 (scale 1.3133): eps = +0, -0 -> +guard; -+ half the guard / scale -> -+guard; the guard / scale: the guard to a
        # rounding from either branch; 1.5 guard / scale: passes through
        s1 = float(np.log1p(np.exp(1.0)))
        at["where_floor"] = []
        for i, ev in enumerate((0.0, -0.0, 0.5 * GUARD / s1, -0.5 * GUARD / s1, GUARD / s1, 1.5 * GUARD / s1, -1.5 * GUARD / s1)):
            r_, d = take() + i // 2, 2 * (i % 2)
            pre[r_, d], pre[r_, D + d], eps[r_, d] = -200.0, F32(1.0) - off, F32(ev)
            at["where_floor"].append((r_, d))
        row += 4
    assert row <= M, c["name"]
    return at


@functools.lru_cache(maxsize=None)
def ga_data(name):
    """the float32 inputs of a case (numpy), where what is planted sits, the stored loc / scale of the backward"""
    c = GA[name]
    rng = np.random.default_rng(_seed(name))
    M, D = c["M"], c["D"]
    d = dict(case=c)
    d["pre"] = rng.standard_normal((M, 2 * D)).astype(F32) * F32(1.5 if c["loc_mode"] == 1 else 1.0)
    d["eps"] = rng.standard_normal((M, D)).astype(F32)
    d["planted"] = _plant(c, d["pre"], d["eps"], rng)
    for k in ("dsample", "dsample2"):
        d[k] = rng.standard_normal((M, D)).astype(F32)
    d["dkl_row"] = rng.standard_normal(M).astype(F32)
    t = gauss_terms64(d["pre"], d["eps"], D, c["loc_mode"], c["offset"], c["prior4"], guard=c["guard"])
    d["loc32"], d["scale32"] = t["loc"].astype(F32), t["scale"].astype(F32)             # what the forward stores: one rounding
    assert np.isfinite(t["kl_row"]).all() and (t["scale"] > 0).all(), name
    if c["guard"] > 0:
        v = t["loc"] + t["scale"] * d["eps"].astype(np.float64)
        planted = np.zeros((M, D), bool)
        for r_, dd in sum(d["planted"].values(), []):
            planted[r_, dd] = True
        # nothing unplanted near a threshold of the guard: a float32 value on the other side of one than its float64 value
        floorable = ~planted & (c["loc_mode"] == 1) & ((np.arange(D) & 1) == 0)[None]
        assert (np.abs(np.abs(v[floorable]) - GUARD) > 0.1 * GUARD).all() and (np.abs(t["scale"][~planted] / GUARD - 1) > 0.1).all(), name
    return d


def ga_bwd_inputs(d, opt):
    has_ds, has_ds2, has_dkl, dkl_scale = BWD_OPTS[opt]
    return dict(eps=d["eps"] if (has_ds or has_ds2) else None, dsample=d["dsample"] if has_ds else None,
                dsample2=d["dsample2"] if has_ds2 else None, dkl_row=d["dkl_row"] if has_dkl else None, dkl_scale=dkl_scale)


@functools.lru_cache(maxsize=None)
def ga_fwd_ref(name):
    d = ga_data(name)
    c = d["case"]
    loc, scale, sample, kl = gauss64(torch.from_numpy(d["pre"]).double(), torch.from_numpy(d["eps"]).double(), c["D"], c["loc_mode"],
                                     c["offset"], c["prior4"], c["guard"])
    t = gauss_terms64(d["pre"], d["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], guard=c["guard"])
    return dict(loc=loc.numpy(), scale=scale.numpy(), sample=sample.numpy(), kl_row=kl.numpy(), terms=t)


@functools.lru_cache(maxsize=None)
def ga_bwd_ref(name, opt):
    """-> (dpre64 by autograd, S_dpre, dpre64 by hand at the float64 loc / scale)"""
    d = ga_data(name)
    c = d["case"]
    kw = ga_bwd_inputs(d, opt)
    ref = gauss_bwd64(d["pre"], kw["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], kw["dsample"], kw["dsample2"], kw["dkl_row"],
                      kw["dkl_scale"], c["guard"])
    t = gauss_terms64(d["pre"], kw["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], dsample=kw["dsample"], dsample2=kw["dsample2"],
                      dkl_row=kw["dkl_row"], dkl_scale=kw["dkl_scale"], guard=c["guard"])
    return ref, t["S_dpre"], t["dpre"]


# the stored scale of the backward at / under / over the guard (s <= guard decides): rows of (scale, the gradient passes)
def guard_scales():
    g_ = F32(GUARD)
    return ((g_, False), (np.nextafter(g_, F32(0)), False), (np.nextafter(g_, F32(1)), True))


GA_DEFECTS = ("dsp_no_offset", "parity", "no_ds2", "tanh_even", "no_dkl_scale", "nan_kept")


def ga_defect(name, opt, defect):
    """dpre64 of the case with the defect planted"""
    d = ga_data(name)
    c = d["case"]
    kw = ga_bwd_inputs(d, opt)
    if defect in ("dsp_no_offset", "tanh_even"):
        return gauss_terms64(d["pre"], kw["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], dsample=kw["dsample"],
                             dsample2=kw["dsample2"], dkl_row=kw["dkl_row"], dkl_scale=kw["dkl_scale"], guard=c["guard"], defect=defect)["dpre"]
    return gauss_bwd64(d["pre"], kw["eps"], c["D"], c["loc_mode"], c["offset"], c["prior4"], kw["dsample"], kw["dsample2"], kw["dkl_row"],
                       kw["dkl_scale"], c["guard"], defect)


def nvil_inputs(B=70, n_parts=3, n_kl=4, M=1):
    """the riders of air_gauss_sample_bwd_nvil: importance-weight shares, baseline, log q(n), the moving-average block, KL shares"""
    rng = np.random.default_rng(77)
    return dict(imp_parts=(rng.uniform(0, 1, (n_parts, B)) * np.array([2000.0, 300.0, 40.0])[:n_parts, None] + 7.0).astype(F32),
                baseline=(rng.standard_normal(B) * 10).astype(F32), logp=(-rng.uniform(0, 3, B)).astype(F32),
                ema=np.array([800.0, 9.0, 0.9, 1.0], F32), kl_parts=rng.uniform(0, 5, (n_kl, M)).astype(F32))


# ===============================================================================================================
# Op. the optimiser
# ===============================================================================================================
HYPER = {                                   # lr0, lr_mult_tail, decay, momentum, eps, grad_scale
    "script": dict(lr=1e-3, tail=0.25, decay=0.9, momentum=0.9, eps=1e-10, gscale=1.0),
    "momentum0": dict(lr=1e-3, tail=0.25, decay=0.9, momentum=0.0, eps=1e-10, gscale=1.0),
    "decay08": dict(lr=1e-3, tail=0.25, decay=0.8, momentum=0.9, eps=1e-6, gscale=1.0),
    "gscale05": dict(lr=1e-3, tail=0.25, decay=0.9, momentum=0.9, eps=1e-10, gscale=0.5),
    "tail10": dict(lr=1e-3, tail=10.0, decay=0.9, momentum=0.9, eps=1e-10, gscale=1.0),
}
BUFS = ("p", "g", "ms", "mg", "mom")


def lr_vector(n, n_model, h, per_float4=False):
    """the learning rate of every element as the kernels form it: lr0 below n_model, float32(lr0 * lr_mult_tail) from it on.
    Defect per_float4: the boundary applied to whole float4 (right only when n_model % 4 == 0)"""
    lr0 = F32(h["lr"])
    i = np.arange(n)
    if per_float4:
        i = i & ~3
    return np.where(i < n_model, lr0, lr0 * F32(h["tail"])).astype(F32)


def rmsprop32(p, g, ms, mg, mom, lr, h, centred=True, defect=None):
    """rmsprop_elem (csrc/optimizer_device.h) in numpy float32, one rounding per operation, in the kernel's order: lr per element
    (lr_vector).  -> p, ms, mg, mom.  Defects: "fma_msi" (the first product of msi, decay * ms, fused into the sum: fma(decay, ms, (1 - decay) gi gi)), "uncentred" (the denominator
    without mg^2), "eps_in_square" (eps added to mg before the square instead of to the difference)"""
    with np.errstate(all="ignore"):
        p, g, ms, mg, mom, lr = (np.asarray(t, F32) for t in (p, g, ms, mg, mom, lr))
        decay, momentum, eps = F32(h["decay"]), F32(h["momentum"]), F32(h["eps"])
        gi = g * F32(h["gscale"])
        om = F32(1) - decay
        if defect == "fma_msi":
            msi = (np.float64(decay) * ms.astype(np.float64) + (om * gi * gi).astype(np.float64)).astype(F32)
        else:
            msi = decay * ms + om * gi * gi
        mgi = decay * mg + om * gi
        if not centred or defect == "uncentred":
            den = msi + eps
        elif defect == "eps_in_square":
            den = msi - (mgi + eps) * (mgi + eps)
        else:
            den = msi - mgi * mgi + eps
        mo = momentum * mom + lr * gi / np.sqrt(den)
        out = (p - mo, msi, mgi, mo)
        assert all(t.dtype == F32 for t in out)
        return out


def rmsprop64(p, g, ms, mg, mom, lr, h, centred=True):
    """the update in float64 on the float32 inputs (lr: lr_vector's float32 values) -> p, ms, mg, mom"""
    d, m, e, s = (FC.f32v(h[k]) for k in ("decay", "momentum", "eps", "gscale"))
    p, g, ms, mg, mom, lr = (np.asarray(t, np.float64) for t in (p, g, ms, mg, mom, lr))
    gi = g * s
    msi = d * ms + (1.0 - d) * gi * gi
    mgi = d * mg + (1.0 - d) * gi
    mo = m * mom + lr * gi / np.sqrt((msi - mgi * mgi if centred else msi) + e)
    return p - mo, msi, mgi, mo


def epilogue_form(n, n_model, off=()):
    """the rule of air_step_epilogue_shadow: the float4 form only for n_total, n_model multiples of 4 and every buffer on a 16-byte
    boundary -> "vec" | "scalar" """
    return "vec" if n % 4 == 0 and n_model % 4 == 0 and not off else "scalar"


def epilogue_items(n, n_model, off=()):
    return n // 4 if epilogue_form(n, n_model, off) == "vec" else n


OP = {}


def _op(name, entry, n, n_model=None, hyper="script", state="ordinary", off=(), counters="both", shadow=False, lo=None, hi=None):
    """entry: "epilogue" | "rmsprop" (air_rmsprop, centred) | "rmsprop_centered" | "rmsprop_plain" | "rider"
    (air_lstm_pointwise_bwd_opt, slice [lo, hi)); state: "ordinary" | "planted" (near-constant gradient: NaN in part of the elements);
    counters: "both" | "no_gstep" | "no_rng" | "none"; off: the buffers 4 bytes past a 16-byte boundary"""
    assert name not in OP
    if n_model is None:                         # the stand-alone update has one learning rate, lr0 * lr_mult: every element is "tail"
        n_model = 0
    OP[name] = dict(name=name, entry=entry, n=n, n_model=n_model, hyper=hyper, state=state, off=tuple(off),
                    counters=counters, shadow=shadow, lo=lo, hi=hi)


for _n in (1, 3, 4, 4099, 4100):
    for _nm in sorted({0, 2, 4, 6, _n - 4, _n}):
        if 0 <= _nm <= _n:
            _op(f"Op_epi_n{_n}_m{_nm}", "epilogue", _n, _nm, hyper="tail10" if _n > 4 else "script", shadow=(_nm % 2 == 0))
for _h in HYPER:
    _op(f"Op_epi_vec_{_h}", "epilogue", 4100, 2048, hyper=_h)
    _op(f"Op_epi_scalar_{_h}", "epilogue", 4099, 2050, hyper=_h)
    _op(f"Op_rmsprop_{_h}", "rmsprop", 4099, hyper=_h)
for _b in BUFS:
    _op(f"Op_epi_off_{_b}", "epilogue", 4100, 2048, hyper="tail10", off=(_b,), shadow=True)
for _cn in ("no_gstep", "no_rng", "none"):
    _op(f"Op_epi_counters_{_cn}", "epilogue", 4100, 2048, counters=_cn)
_op("Op_epi_planted_vec", "epilogue", 4100, 2048, state="planted", shadow=True)
_op("Op_epi_planted_scalar", "epilogue", 4099, 2050, state="planted", shadow=True)
_op("Op_rmsprop_planted", "rmsprop", 4099, state="planted")
_op("Op_rmsprop_centered_entry", "rmsprop_centered", 4099, hyper="decay08")
_op("Op_epi_scalar_strided", "epilogue", CAP_ITEMS + 3, CAP_ITEMS - 2, hyper="tail10", shadow=True)           # 524 291 items
_op("Op_epi_vec_strided", "epilogue", 4 * CAP_ITEMS + 4, 4 * CAP_ITEMS, hyper="tail10", shadow=True)          # 2 097 156 floats
_op("Op_rmsprop_strided", "rmsprop", CAP_ITEMS + 3, hyper="decay08")
for _n in (1, 3, 4):
    _op(f"Op_rmsprop_n{_n}", "rmsprop", _n)
for _n in (1, 3, 4, 4099, CAP_ITEMS + 3, 4 * CAP_ITEMS + 4):
    _op(f"Op_plain_n{_n}", "rmsprop_plain", _n, hyper="decay08" if _n == 4099 else "script")
_op("Op_plain_momentum0", "rmsprop_plain", 4099, hyper="momentum0")
_op("Op_rider", "rider", 4100, 2048, hyper="tail10", lo=4, hi=4096)
_op("Op_rider_planted", "rider", 4100, 2048, state="planted", lo=0, hi=4100)
_op("Op_rider_tail_only", "rider", 4100, 0, hyper="gscale05", lo=8, hi=4000)
OP_STRIDED = ("Op_epi_scalar_strided", "Op_epi_vec_strided", "Op_rmsprop_strided", f"Op_plain_n{CAP_ITEMS + 3}")
GSTEP0, RNG0, RNG_INC = 41, (0x1234567890ABCDEF, 2 ** 64 - 5), 2 ** 32 + 7        # the Philox offset wraps: (2^64 - 5) + 2^32 + 7 = 2^32 + 2
NAN_SHARE = (0.10, 0.90)


def i64(v):
    """a 64-bit pattern as the int64 a torch tensor holds"""
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


@functools.lru_cache(maxsize=None)
def op_data(name):
    """the float32 state of a case (numpy) and the restatement's result"""
    c = OP[name]
    rng = np.random.default_rng(_seed(name))
    n, h = c["n"], HYPER[c["hyper"]]
    d = dict(case=c, h=h)
    d["g"] = rng.standard_normal(n).astype(F32)
    d["p"] = rng.standard_normal(n).astype(F32)
    if c["state"] == "planted":
        # a gradient that has been constant for long: mg = g, ms = g^2 moved by -3 ... +3 float32 steps, so that ms' - mg'^2 + eps is
        # a rounding remnant of either sign; the square root of a negative one is NaN (the reference's arithmetic: match, don't clamp)
        d["mg"] = d["g"].copy()
        sq = (d["g"] * d["g"]).astype(F32)
        d["ms"] = (sq.view(np.int32) + rng.integers(-3, 4, n).astype(np.int32)).view(F32)
        d["mom"] = np.zeros(n, F32)
    else:
        d["ms"] = (rng.uniform(0, 1, n) + 1.0).astype(F32)
        d["mg"] = (rng.standard_normal(n) * 0.1).astype(F32)
        d["mom"] = (rng.standard_normal(n) * 0.01).astype(F32)
    centred = c["entry"] != "rmsprop_plain"
    lr = lr_vector(n, c["n_model"], h)
    lo, hi = (0, n) if c["lo"] is None else (c["lo"], c["hi"])
    new = rmsprop32(*(d[k] for k in BUFS), lr, h, centred)
    d["lr"], d["span"] = lr, (lo, hi)
    d["ref32"] = {}
    for k, t in zip(("p", "ms", "mg", "mom"), new):
        full = d[k].copy()
        full[lo:hi] = t[lo:hi]
        d["ref32"][k] = full
    return d


def op_ref64(d, centred=True):
    new = rmsprop64(*(d[k] for k in BUFS), d["lr"], d["h"], centred)
    return dict(zip(("p", "ms", "mg", "mom"), new))


OP_DEFECTS = ("per_float4", "uncentred", "eps_in_square", "fma_msi")


def op_defect(name, defect):
    """the restatement's result on the case with the defect planted -> dict p, ms, mg, mom"""
    d = op_data(name)
    c = d["case"]
    lr = lr_vector(c["n"], c["n_model"], d["h"], per_float4=(defect == "per_float4"))
    new = rmsprop32(*(d[k] for k in BUFS), lr, d["h"], True, None if defect == "per_float4" else defect)
    return dict(zip(("p", "ms", "mg", "mom"), new))


# ---- air_l2_grad_add ---------------------------------------------------------------------------------------------------------------
L2_MAX_RANGES = 32
L2_WEIGHT = 1e-3
L2_TOL = (2.0 ** -23, 1e-9)                 # the bar of tests/test_fold_kernels.py: one float32 rounding of the float64 value, fused or not
L2 = {
    # 32 ranges (the maximum) of uneven lengths with gaps between them, unaligned starts
    "L2_32_ranges": dict(n=4099, ranges=tuple((127 * k + (k % 3), 127 * k + (k % 3) + 5 + 3 * k) for k in range(32)), status=0),
    "L2_33_ranges": dict(n=4099, ranges=tuple((100 * k, 100 * k + 7) for k in range(33)), status=E_SHAPE),
    "L2_lo_above_hi": dict(n=1000, ranges=((4, 300), (500, 499)), status=E_SHAPE),
    "L2_strided": dict(n=CAP_ITEMS + 40, ranges=((3, 3), (7, CAP_ITEMS + 12), (CAP_ITEMS + 20, CAP_ITEMS + 33)), status=0),    # empty first; 524 293 elements
    "L2_one": dict(n=9, ranges=((5, 6),), status=0),
    "L2_zero_ranges": dict(n=9, ranges=(), status=E_SHAPE),
}


@functools.lru_cache(maxsize=None)
def l2_data(name):
    c = L2[name]
    rng = np.random.default_rng(_seed(name))
    g, p = rng.standard_normal(c["n"]).astype(F32), rng.standard_normal(c["n"]).astype(F32)
    inside = np.zeros(c["n"], bool)
    if c["status"] == 0:
        for lo, hi in c["ranges"]:
            assert not inside[lo:hi].any(), name
            inside[lo:hi] = True
    return dict(case=c, g=g, p=p, inside=inside, ref64=g.astype(np.float64) + FC.f32v(L2_WEIGHT) * p.astype(np.float64))


# ===============================================================================================================
# Bf. the bf16 casts
# ===============================================================================================================
def bf16_rne(bits):
    """float32 bit patterns (uint32) -> bf16 bit patterns (uint16) by integer round-to-nearest-even; valid for every non-NaN input"""
    b = np.asarray(bits, np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_truncate(bits):
    return (np.asarray(bits, np.uint32) >> 16).astype(np.uint16)


def is_nan32(bits):
    b = np.asarray(bits, np.uint32)
    return ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)


def is_nan16(h):
    h = np.asarray(h, np.uint16)
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)


def bf16_mismatches(src_bits, out16, rounding=bf16_rne):
    """-> number of elements of out16 that are not the cast of src_bits: bits for a non-NaN source, any NaN for a NaN source"""
    src_bits, out16 = np.asarray(src_bits, np.uint32).ravel(), np.asarray(out16, np.uint16).ravel()
    assert src_bits.shape == out16.shape
    nan = is_nan32(src_bits)
    return int((np.where(nan, ~is_nan16(out16), out16 != rounding(src_bits))).sum())


NAN_PATTERNS = (0x7F800001, 0x7FFFFFFF, 0x7FC00000, 0xFF800001, 0xFFC12345)
CRAFTED = (
    0x3F808000,     # tie, even kept mantissa: stays 0x3F80
    0x3F818000,     # tie, odd kept mantissa: up to 0x3F82
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,                 # one ulp either side of each tie
    0x3FFF8000,     # tie that carries into the exponent: 0x4000
    0xBFFF8000, 0x00000000, 0x80000000,
    0x00000001,     # the smallest subnormal
    0x00008000, 0x00018000,                                         # subnormal ties: to 0x0000 (even) and 0x0002
    0x007FFFFF,     # the largest subnormal: rounds up to the smallest normal 0x0080
    0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,                             # below the last tie; the tie and FLT_MAX: round to inf
    0x7F800000, 0xFF800000,
) + NAN_PATTERNS


@functools.lru_cache(maxsize=None)
def bf16_values(n_random=4099):
    """uint32 patterns: the crafted list laid out so that each value lands in every position of a float4 (the list four times, each copy
    one element further, padded with 1.0), then n_random random finite patterns; the length is a multiple of 4"""
    rng = np.random.default_rng(16)
    parts = []
    for shift in range(4):
        parts.append(np.array((0x3F800000,) * shift + CRAFTED + (0x3F800000,) * ((-(shift + len(CRAFTED))) % 4), np.uint32))
    rnd = rng.standard_normal(n_random).astype(F32) * np.exp(rng.uniform(-20, 20, n_random)).astype(F32)
    parts.append(rnd.view(np.uint32))
    v = np.concatenate(parts)
    v = np.concatenate([v, np.full((-len(v)) % 4, 0x3F800000, np.uint32)])
    pos = {(int(x), i % 4) for i, x in enumerate(v[:sum(len(p) for p in parts[:4])])}
    assert all((c, k) in pos for c in CRAFTED for k in range(4))
    return v


# entry, n (None: all of bf16_values), source 4 bytes off, destination 2 bytes off -> the kernel
BF = {
    "Bf_vec": dict(entry="cast", tail=0, src_off=False, dst_off=False, kernel="f32_to_bf16_vec_kernel"),
    "Bf_scalar_tail": dict(entry="cast", tail=3, src_off=False, dst_off=False, kernel="f32_to_bf16_kernel"),          # n % 4 == 1
    "Bf_src_off": dict(entry="cast", tail=0, src_off=True, dst_off=False, kernel="f32_to_bf16_kernel"),
    "Bf_dst_off": dict(entry="cast", tail=0, src_off=False, dst_off=True, kernel="f32_to_bf16_kernel"),
    "Bf_shadow_vec": dict(entry="shadow", tail=0, src_off=False, dst_off=False, kernel="step_epilogue_kernel<true>"),
    "Bf_shadow_scalar": dict(entry="shadow", tail=3, src_off=False, dst_off=False, kernel="step_epilogue_kernel<false>"),
    "Bf_prologue_cvt": dict(entry="cvt", tail=0, src_off=False, dst_off=False, kernel="step_prologue_cvt_kernel"),
}
BF_STRIDED_N = 4 * CAP_ITEMS + 4            # the vector cast strides above 2 097 152 floats


def bf_source(name):
    v = bf16_values()
    return v[:len(v) - BF[name]["tail"]] if BF[name]["tail"] else v


# ===============================================================================================================
# Ut. utilities
# ===============================================================================================================
UT_SIZES = (1, 255, 257, CAP_ITEMS + 3)
AXPBY_RTOL = 2.0 ** -23                     # alpha a + beta b with one rounding per operation or fused: within 2^-23 relative ...
COLSUM = ((1, 1), (7, 255), (5, 257), (3, CAP_ITEMS + 3))          # (M, N), ld = N + 3


def axpby_inputs(n, with_b):
    """same-signed summands, so that 2^-23 of the RESULT covers the rounding of each summand too"""
    rng = np.random.default_rng(n + int(with_b))
    return rng.uniform(0.5, 1.5, n).astype(F32), (rng.uniform(0.5, 1.5, n).astype(F32) if with_b else None), 1.7, 0.3


def colsum32(x):
    """the float32 column sums with the rows added in order from 0.f"""
    s = np.zeros(x.shape[1], F32)
    for m in range(x.shape[0]):
        s = (s + x[m]).astype(F32)
    return s


# ===============================================================================================================
# every kernel instantiation behind these entries, and the cases that name each
# ===============================================================================================================
KERNELS = ("gauss_fwd_kernel", "gauss_bwd_kernel", "gauss_bwd_nvil_kernel", "normal_kl_fwd_kernel", "normal_kl_bwd_kernel",
           "heads_fwd_kernel<8>", "heads_fwd_kernel<32>", "heads_bwd_kernel<8>", "heads_bwd_kernel<32>",
           "rmsprop_kernel<true>", "rmsprop_kernel<false>", "step_epilogue_kernel<true>", "step_epilogue_kernel<false>",
           "lstm_pw_bwd_opt_kernel", "f32_to_bf16_kernel", "f32_to_bf16_vec_kernel", "step_prologue_cvt_kernel", "l2_grad_kernel",
           "fill_kernel", "axpby_kernel", "tile_rows_kernel", "colsum_kernel")


def kernels_named():
    """kernel -> the cases (or case families) of this module that launch it, by the launch rules restated here"""
    named = {k: [] for k in KERNELS}
    for n_, c in GA.items():
        named["gauss_fwd_kernel"].append(n_)
        named["normal_kl_fwd_kernel"].append(n_)
        if c["bwd"]:
            named["gauss_bwd_kernel"].append(n_)
        if c["kl_bwd"]:
            named["normal_kl_bwd_kernel"].append(n_)
    named["gauss_bwd_nvil_kernel"] += list(GA_STRIDED_BWD)
    for T, B in HEADS_TB:
        named["heads_fwd_kernel<%d>" % (8 if T <= 8 else 32)].append((T, B))
        named["heads_bwd_kernel<%d>" % (8 if T <= 8 else 32)].append((T, B))
    for n_, c in OP.items():
        if c["entry"] == "epilogue":
            named["step_epilogue_kernel<%s>" % ("true" if epilogue_form(c["n"], c["n_model"], c["off"]) == "vec" else "false")].append(n_)
        elif c["entry"] == "rider":
            named["lstm_pw_bwd_opt_kernel"].append(n_)
        else:
            named["rmsprop_kernel<%s>" % ("false" if c["entry"] == "rmsprop_plain" else "true")].append(n_)
    for n_, c in BF.items():
        named[c["kernel"]].append(n_)
    named["l2_grad_kernel"] += [n_ for n_, c in L2.items() if c["status"] == 0]
    for k in ("fill_kernel", "axpby_kernel", "tile_rows_kernel"):
        named[k] += list(UT_SIZES)
    named["colsum_kernel"] += list(COLSUM)
    return named
