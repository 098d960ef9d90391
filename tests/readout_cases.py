"""Cases, float64 references, numpy float32 restatements (one rounding per operation), bounds and planted defects for the kernel-level
tests of the evaluation and parse read-outs: groups Iw (air_iw_logweight, air_iw_logposterior, air_iw_reduce + the running totals), Pp
(air_particle_select, air_particle_spread), Gn (air_prior_latents, air_observe) and Ps (air_parse_objects, air_parse_render).  tests/test_readout_kernels.py runs them on the
device one launch at a time, tests/test_readout_cases_host.py holds this module on the CPU.

Bounds are elementwise, CONST * 2^-24 * S with S the magnitudes of the element's summands (for a K-term float32 sum: what the
lane-strided sum of that many terms costs, DEPTH(K) roundings of the sum of magnitudes).  Every CONST is four times the worst ratio of
the float32 restatement of the kernel's own order, rounded up (RESTATEMENT_SHARE = 0.25, the project's rule); the measured ratios are
in RESTATEMENT_RATIO and DESIGN.md, and the host test fails when the restatement leaves its share.

Windows, sentinels, the transforms of the warp groups and the Philox restatement come from tests/warp_cases.py and tests/fold_cases.py."""
import functools
import zlib

import numpy as np
import torch

import fold_cases as FC
import warp_cases as WC
from attend_cases import SENTINEL
from warp_cases import DEFECT_MARGIN, NAN, RESTATEMENT_SHARE, out_win, surroundings_intact  # noqa: F401  (re-exported to the tests)

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
INT_FILL = -77777                 # what surrounds an integer operand (integers have no NaN)
INT_PRIMER = -999                 # what an integer output holds before the launch
HALF_LOG_2PI = F32(0.91893853320467274178)
QNAN_BITS = 0x7fc00000

# CONST of every bound, and the worst float32-restatement ratio (error / (2^-24 S)) it is four times of, measured on the CPU by
# tests/test_readout_cases_host.py::test_restatements_keep_their_share (which prints them with -s)
RESTATEMENT_RATIO = {"logw": 0.918, "logq": 1.143, "iw_bound": 0.642, "elbo": 0.201, "ess": 0.174, "q_n": 0.172, "latents": 1.528}
CONST = {"logw": 4.0, "logq": 5.0, "iw_bound": 3.0, "elbo": 1.0, "ess": 1.0, "q_n": 1.0, "latents": 7.0}
SPREAD_F64_CONST = 2.0            # the float64 term of the spread's bound: CONST * 2^-53 * S, four times the lane-order restatement's ratio
SPREAD_F64_RATIO = 0.410


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


class Win(WC.Win):
    """warp_cases.Win with the lead given in elements (`off` = 1: 4 bytes off a 16-byte boundary for float32, 2: 8 bytes) and any dtype"""

    def __init__(self, shape, off=0, fill=NAN, inner=None, dtype=torch.float32):
        self.shape, self.lead = tuple(shape), 8 + int(off)
        self.n = int(np.prod(self.shape))
        self.parent = torch.full((self.lead + self.n + 8,), fill, dtype=dtype)
        self.v = self.parent[self.lead:self.lead + self.n].view(self.shape)
        if inner is not None:
            self.v.fill_(inner)


def in_win(values, off=0):
    """an operand: a window of a NaN parent (integers: of an INT_FILL parent)"""
    v = torch.as_tensor(np.ascontiguousarray(values))
    win = Win(v.shape, off, NAN if v.dtype.is_floating_point else INT_FILL, dtype=v.dtype)
    win.v.copy_(v)
    return win


def out_window(shape, off=0, dtype=torch.float32):
    """an output: a NaN-primed (integers: INT_PRIMER) window of a SENTINEL parent"""
    return Win(shape, off, SENTINEL, NAN if dtype.is_floating_point else INT_PRIMER, dtype=dtype)


def same_bits(a, b):
    """number of elements whose bits differ (any NaN equals any NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != "f":
        return int((a != b).sum())
    ia = a.view(np.int32 if a.dtype == F32 else np.int64)
    ib = b.view(ia.dtype)
    return int(((ia != ib) & ~(np.isnan(a) & np.isnan(b))).sum())


def classes(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, position by position"""
    x = np.asarray(x, F64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def depth(K):
    """additions on the longest path of a sum of K terms strided over 64 lanes and joined by a butterfly"""
    return -(-int(K) // 64) + 6


def butterfly(s):
    """wave_sum_all on the 64 per-lane values (trailing axis): off = 32 .. 1, every lane adds its partner; lane 0's total"""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ off]
    return s[..., 0]


def lane_sums(terms, dtype):
    """[..., K] -> the 64 per-lane sums of `for (k = lane; k < K; k += 64) s += terms[k]` in `dtype`, starting at 0"""
    terms = np.asarray(terms, dtype)
    K = terms.shape[-1]
    P = -(-K // 64)
    pad = np.zeros(terms.shape[:-1] + (P * 64,), dtype)
    pad[..., :K] = terms
    pad = pad.reshape(terms.shape[:-1] + (P, 64))
    valid = (np.arange(P * 64) < K).reshape(P, 64)
    s = np.zeros(terms.shape[:-1] + (64,), dtype)
    for p in range(P):
        s = np.where(valid[p], s + pad[..., p, :], s)
    return s


# ---------------------------------------------------------------------------------------------------------------
# Iw: the row kernels (iw_logweight_kernel<V>, iw_logposterior_kernel<V>: one lane layout, one table, one set of inputs)
# ---------------------------------------------------------------------------------------------------------------
IW_PRIORS = {"fixed": (0.3, 1.5, 0.6, 0.4, -0.2, 0.7), "centred": (0.0, 1.0, 0.5, 0.5, NAN, 0.7)}
LATENTS = ("what", "what_loc", "what_scale")


def iw_vec(A, off):
    """the launch rule of air_iw_logweight / air_iw_logposterior / air_prior_latents: `off` = the float offsets of the A-wide operands"""
    bits = 0
    for o in off.values():
        bits |= 4 * o
    return 4 if A % 4 == 0 and bits & 15 == 0 else (2 if A % 2 == 0 and bits & 7 == 0 else 1)


def _iw(T, R, K, A, prior, norm, rows=None, off=None, data=None, reaches=""):
    off = dict(off or {})
    return dict(T=T, R=R, K=K, A=A, prior=prior, norm=norm, rows=dict(rows or {}), off=off, data=data, V=iw_vec(A, off), reaches=reaches)


_P5 = {0: "half", 1: "nonmono", 2: "nan_tail", 3: "logp_ninf", 4: "bigz"}
IW_ROWS = {
    "Iw_1x1x1x1": _iw(1, 1, 1, 1, "fixed", 0, reaches="the smallest launch"),
    "Iw_3x7x1x50": _iw(3, 7, 1, 50, "centred", 1, {2: "half", 3: "nonmono", 4: "nan_tail", 5: "bigz", 6: "scale0_ne"},
                       reaches="V = 2; three live waves in the last workgroup; 75 items: a second pass of the lane loop"),
    "Iw_5x6x3x12": _iw(5, 6, 3, 12, "fixed", 1, {4: "prior0", 5: "scale0_eq"}, reaches="V = 4"),
    "Iw_32x9x3x8": _iw(32, 9, 3, 8, "centred", 0, {4: "scale0_ne", 5: "scale0_eq", 6: "bigz", 7: "prior0", 8: "logp_ninf"},
                       reaches="n = 0, 1, 31, 32; 64 items: exactly one pass"),
    "Iw_32x9x3x12": _iw(32, 9, 3, 12, "fixed", 1, {4: "nonmono", 5: "half", 6: "bigz", 7: "prior0", 8: "nan_tail"}, reaches="96 items"),
    "Iw_3x5x5x52": _iw(3, 5, 5, 52, "centred", 1, _P5, reaches="V = 4 at A = 52"),
    "Iw_2x257x1x5": _iw(2, 257, 1, 5, "fixed", 0, {100: "bigz", 101: "logp_ninf", 102: "scale0_ne", 103: "half"},
                        reaches="65 workgroups, the last with one live wave; odd A: V = 1"),
    "Iw_3x5x1x6": _iw(3, 5, 1, 6, "fixed", 1, _P5, reaches="A = 6, aligned: V = 2"),
}
for _name in LATENTS:
    for _o in (1, 2):
        IW_ROWS[f"Iw_3x5x5x52_{_name}_{4 * _o}B"] = _iw(3, 5, 5, 52, "centred", 1, _P5, off={_name: _o}, data="Iw_3x5x5x52",
                                                       reaches=f"V = {1 if _o == 1 else 2} by the alignment of {_name}")
for _o in (1, 2):
    IW_ROWS[f"Iw_3x5x5x52_all_{4 * _o}B"] = _iw(3, 5, 5, 52, "centred", 1, _P5, off={k: _o for k in LATENTS}, data="Iw_3x5x5x52",
                                              reaches=f"the same values on V = {1 if _o == 1 else 2}")
IW_BIT_PEERS = {1: "Iw_3x5x5x52_all_4B", 2: "Iw_3x5x5x52_all_8B"}          # V -> the launch every misaligned launch on V must equal


@functools.lru_cache(maxsize=None)
def iw_data(name):
    """float32 inputs of a row case (shared by the rows that differ in alignment only) -> dict of numpy arrays + n [R] + the table"""
    c = IW_ROWS[name]
    if c["data"]:
        return iw_data(c["data"])
    T, R, A = c["T"], c["R"], c["A"]
    rng = np.random.default_rng(_seed(name))
    zi = 2 if T >= 3 else None                                              # the table entry that is exactly 0
    table = rng.uniform(0.05, 1.0, T + 1)                                   # does not sum to 1
    if zi is not None:
        table[zi] = 0.0
    ns = np.array(([T, 0, 1, max(T - 1, 0)] + list(rng.integers(0, T + 1, max(R - 4, 0))))[:R])
    if zi is not None:
        ns[ns == zi] = zi + 1
    kinds = c["rows"]
    for r, kind in kinds.items():
        ns[r] = {"prior0": zi, "half": 1, "nonmono": 1, "nan_tail": 0}.get(kind, T)
    pres = (np.arange(T)[:, None] < ns[None, :]).astype(F32)
    for r, kind in kinds.items():
        if kind == "half":
            pres[1:, r] = 1.0
            pres[1, r] = 0.5                                                # not > 0.5: absent, whatever follows
        elif kind == "nonmono":
            pres[:, r] = (np.arange(T) % 2 == 0)                            # (1, 0, 1, ...): one leading one
        elif kind == "nan_tail":
            pres[1:, r] = NAN                                               # behind the first absent step nothing is read for its value

    def normal(*shape):
        return rng.standard_normal(shape).astype(F32)

    d = {}
    for base, width in (("what", A), ("where", 4)):
        loc, scale = normal(T, R, width), np.exp(F32(0.5) * normal(T, R, width))
        d[base], d[base + "_loc"], d[base + "_scale"] = loc + scale * normal(T, R, width), loc, scale
    d["rec"] = rng.uniform(100.0, 800.0, R).astype(F32)
    d["logp"] = (-rng.uniform(0.0, T, R)).astype(F32)
    for r, kind in kinds.items():
        if kind == "scale0_ne":
            d["what_scale"][0, r, A // 2] = 0.0
        elif kind == "scale0_eq":
            d["where_scale"][0, r, 2] = 0.0
            d["where"][0, r, 2] = d["where_loc"][0, r, 2]
        elif kind == "bigz":                                                # |z| from 1e2 to 1e4: z * z far below float32's overflow
            z = np.where(np.arange(A) % 2 == 0, 1.0, -1.0) * np.logspace(2, 4, A)
            d["what"][0, r] = d["what_loc"][0, r] + d["what_scale"][0, r] * z.astype(F32)
            d["where"][0, r, 1] = d["where_loc"][0, r, 1] + d["where_scale"][0, r, 1] * F32(1e4)
        elif kind == "logp_ninf":
            d["logp"][r] = -np.inf
    absent = np.arange(T)[:, None] >= ns[None, :]
    for k in ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale"):
        d[k][absent] = NAN                                                  # a mask error is a NaN, not a tolerance
    d.update(presence=pres, n=ns.astype(np.int32), table=table, zi=zi)
    return d


def iw_ref64(name, defect=None):
    """float64 on the float32 inputs -> dict(logw, logq, n, S_logw, S_logq); `defect`: one of IW_DEFECTS"""
    c, d = IW_ROWS[name], iw_data(name)
    T, R, A = c["T"], c["R"], c["A"]
    pw_loc, pw_scale, ps_loc, ps_scale, ph_loc, ph_scale = (float(F32(v)) for v in IW_PRIORS[c["prior"]])
    n = np.array([int(np.argmin(np.concatenate([d["presence"][:, r] > 0.5, [False]]))) for r in range(R)])
    upto = n + 1 if defect == "step_n_included" else (n - 1 if defect == "step_before_n_dropped" else n)
    mask = (np.arange(T)[:, None] < upto[None, :])[:, :, None]
    out = {}
    with np.errstate(all="ignore"):
        tot_w, tot_q, S_w, S_q = np.zeros(R), np.zeros(R), np.zeros(R), np.zeros(R)
        for base, width in (("what", A), ("where", 4)):
            x, l, s = (d[base + k].astype(F64) for k in ("", "_loc", "_scale"))
            if base == "what":
                p_loc, p_scale = np.full_like(x, pw_loc), np.full_like(x, pw_scale)
            else:
                centred = np.isnan(ph_loc) and defect != "shift_not_centred"
                shift_loc = l if centred else np.full_like(x, 0.0 if np.isnan(ph_loc) else ph_loc)
                even = (np.arange(4) % 2 == 0)[None, None, :]
                p_loc, p_scale = np.where(even, ps_loc, shift_loc), np.where(even, ps_scale, ph_scale) * np.ones_like(x)
            zq, zp = (x - l) / s, (x - p_loc) / p_scale
            lps = 0.0 if defect == "log_p_scale_dropped" else np.log(p_scale)
            ratio = 0.5 * (zq * zq - zp * zp) + (np.log(s) - lps)
            logq = -0.5 * zq * zq - np.log(s) - 0.5 * np.log(2.0 * np.pi)       # (the kernel's constant is this, rounded to float32)
            tot_w += np.where(mask, ratio, 0.0).sum((0, 2))
            tot_q += np.where(mask, logq, 0.0).sum((0, 2))
            S_w += np.where(mask, 0.5 * zq * zq + 0.5 * zp * zp + np.abs(np.log(s)) + np.abs(np.log(p_scale)), 0.0).sum((0, 2))
            S_q += np.where(mask, 0.5 * zq * zq + np.abs(np.log(s)) + float(HALF_LOG_2PI), 0.0).sum((0, 2))
        total = d["table"].sum() if (c["norm"] and defect != "table_not_normalised") else 1.0
        log_prior = np.log(d["table"][n] / total)
        rec, logp = d["rec"].astype(F64), d["logp"].astype(F64)
        out["logw"] = -rec + (log_prior - logp) + tot_w
        out["logq"] = logp + tot_q
        out["S_logw"] = S_w + np.abs(rec) + np.abs(log_prior) + np.abs(logp) + np.abs(out["logw"])
        out["S_logq"] = S_q + np.abs(logp) + np.abs(out["logq"])
    out["n"] = n.astype(np.int32)
    return out


IW_DEFECTS = ("step_n_included", "step_before_n_dropped", "shift_not_centred", "log_p_scale_dropped", "table_not_normalised")


def _ratio32(x, l, c, pl, ps, lps):
    zq, zp = (x - l) / c, (x - pl) / ps
    return F32(0.5) * (zq * zq - zp * zp) + (np.log(c) - lps)


def _logn32(x, l, c):
    z = (x - l) / c
    return F32(-0.5) * (z * z) - np.log(c) - HALF_LOG_2PI


def _row_sum32(what_terms, where_terms, n, AV, V):
    """the lane layout of both row kernels: what_terms [n * AV * V] in (t, i, v) order, where_terms [n, 4]"""
    s = np.zeros(64, F32)
    items = n * AV
    vals = what_terms.reshape(items, V)
    for j0 in range(0, items, 64):
        cnt = min(64, items - j0)
        for v in range(V):
            s[:cnt] = s[:cnt] + vals[j0:j0 + cnt, v]
    for k in range(4):
        s[:n] = s[:n] + where_terms[:, k]
    return butterfly(s)


def iw_restate32(name, V):
    """numpy float32, one rounding per operation, in the lane order of vector width V -> (logw32, logq32)"""
    c, d = IW_ROWS[name], iw_data(name)
    T, R, A = c["T"], c["R"], c["A"]
    pr = [F32(v) for v in IW_PRIORS[c["prior"]]]
    AV = A // V
    centred = np.isnan(pr[4])
    logw, logq = np.empty(R, F32), np.empty(R, F32)
    with np.errstate(all="ignore"):
        l_pw, l_ps, l_ph = np.log(pr[1]), np.log(pr[3]), np.log(pr[5])
        total = 1.0
        if c["norm"]:
            total = 0.0
            for i in range(T + 1):
                total += d["table"][i]
        for r in range(R):
            n = int(d["n"][r])
            x, l, s = (d["what" + k][:n, r, :AV * V].reshape(-1) for k in ("", "_loc", "_scale"))
            wx, wl, ws = (d["where" + k][:n, r] for k in ("", "_loc", "_scale"))
            p_loc = np.stack([np.full(n, pr[2], F32), wl[:, 1] if centred else np.full(n, pr[4], F32),
                              np.full(n, pr[2], F32), wl[:, 3] if centred else np.full(n, pr[4], F32)], 1)
            p_scale = np.array([pr[3], pr[5], pr[3], pr[5]], F32)[None, :]
            l_p = np.array([l_ps, l_ph, l_ps, l_ph], F32)[None, :]
            sw = _row_sum32(_ratio32(x, l, s, pr[0], pr[1], l_pw), _ratio32(wx, wl, ws, p_loc, p_scale, l_p), n, AV, V)
            sq = _row_sum32(_logn32(x, l, s), _logn32(wx, wl, ws), n, AV, V)
            log_prior = np.log(d["table"][n] / total)
            logw[r] = F32(-float(d["rec"][r]) + (log_prior - float(d["logp"][r])) + float(sw))
            logq[r] = F32(float(d["logp"][r]) + float(sq))
    return logw, logq


TINY = 2.0 ** -126                 # the smallest normal float32: a softmax share of 1e-320 in float64 is 0 in float32


def bound(kind, S, const=None):
    """CONST * 2^-24 * S (+ TINY where S > 0)"""
    S = np.asarray(S, F64)
    const = const if const is not None else (float(kind) if not isinstance(kind, str) else CONST[kind])     # (a number: another group's CONST)
    return const * U * S + np.where(S > 0, TINY, 0.0)


def worst_ratio(out, ref, S, kind=None):
    """max |out - ref| / (2^-24 S) over the elements where ref is finite (kind given: over the bound instead); the classes must agree"""
    out, ref, S = np.asarray(out, F64), np.asarray(ref, F64), np.asarray(S, F64)
    assert (classes(out) == classes(ref)).all(), (classes(out), classes(ref))
    fin = np.isfinite(ref)
    err, den = np.abs(out[fin] - ref[fin]), bound(kind, S[fin], 1.0 if kind is None else None)
    assert (err[den == 0] == 0).all()
    nz = den > 0
    return float((err[nz] / den[nz]).max()) if nz.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# Iw: air_iw_reduce (iw_reduce_kernel, iw_accumulate_kernel)
# ---------------------------------------------------------------------------------------------------------------
RED_CASES = {f"Red_K{K}_B{B}_T{T}": dict(K=K, B=B, T=T) for K, B, T in
             [(1, 1, 1), (1, 5, 3), (2, 5, 3), (2, 257, 1), (63, 5, 3), (64, 5, 3), (65, 5, 3), (65, 257, 32), (200, 5, 3), (200, 5, 32),
              (4099, 1, 1), (4099, 5, 3)]}
RED_KINDS = ("wide", "equal", "some_ninf", "outside", "narrow")              # image b is of kind b % 5


@functools.lru_cache(maxsize=None)
def red_data(name):
    """-> logw [B, K] float32 centred at -3000 with a spread of 1000 nats, n [B, K] int32"""
    c = RED_CASES[name]
    K, B, T = c["K"], c["B"], c["T"]
    rng = np.random.default_rng(_seed(name))
    lw = (-3000.0 + rng.uniform(-500.0, 500.0, (B, K))).astype(F32)
    n = rng.integers(0, T + 1, (B, K)).astype(np.int32)
    for b in range(B):
        kind = RED_KINDS[b % 5]
        if kind == "equal":
            lw[b] = F32(-3000.25)
            n[b] = np.where(np.arange(K) % 2 == 0, 0, T)                     # K even: q_n[0] == q_n[T] == 0.5 exactly, an arg-max tie
        elif kind == "some_ninf":
            lw[b, ::3] = -np.inf                                             # weights of exactly 0 (never all of them: K = 1 keeps its one)
            if K == 1:
                lw[b, 0] = F32(-2999.0)
        elif kind == "outside":
            lw[b] = (-3000.0 + rng.uniform(-2.0, 2.0, K)).astype(F32)
            n[b, ::4] = -1                                                   # counted nowhere
            n[b, 1::4] = T + 1
        elif kind == "narrow":
            lw[b] = (-3000.0 + rng.uniform(-2.0, 2.0, K)).astype(F32)
    return dict(logw=lw, n=n)


def red_ref64(lw, n, T, defect=None):
    """float64 logsumexp / mean / softmax on the float32 log-weights (finite maxima only) -> outputs and their S"""
    lw64 = np.asarray(lw, F64)
    B, K = lw64.shape
    with np.errstate(all="ignore"):
        m = lw64.max(1, keepdims=True)
        shift = np.zeros_like(m) if defect == "no_shift" else m
        dlt = lw64 - shift
        w = np.exp(dlt)
        cost = np.where(w > 0, w * (np.abs(np.where(w > 0, dlt, 0.0)) + 2.0), 0.0)    # one rounding of lw - shift, the exponential's two
        s1, s2 = w.sum(1), (w * w).sum(1)
        D = float(depth(K))
        E1 = cost.sum(1) / s1 + D
        E2 = (2.0 * w * cost).sum(1) / s2 + D + 1.0
        out = dict(iw_bound=shift[:, 0] + np.log(s1) - np.log(float(K)), elbo=lw64.sum(1) / K,
                   ess=(s1 / s2 if defect == "ess_s1_over_s2" else s1 * s1 / s2))
        out["S_iw_bound"] = np.abs(m[:, 0]) + np.abs(np.log(s1)) + np.log(float(K)) + np.abs(out["iw_bound"]) + E1
        out["S_elbo"] = np.where(np.isfinite(out["elbo"]), D * np.abs(np.where(np.isfinite(lw64), lw64, 0.0)).sum(1) / K + np.abs(out["elbo"]), 0.0)
        out["S_ess"] = out["ess"] * (2.0 * E1 + E2 + 3.0)
        q, S_q = np.zeros((B, T + 1)), np.zeros((B, T + 1))
        for c in range(T + 1):
            sel = np.asarray(n) == c
            sc = np.where(sel, w, 0.0).sum(1)
            q[:, c] = sc / s1
            S_q[:, c] = np.where(sc > 0, q[:, c] * (np.where(sel, cost, 0.0).sum(1) / np.where(sc > 0, sc, 1.0) + D + E1 + 1.0), 0.0)
        out["q_n"], out["S_q_n"] = q, S_q
    return out


def red_restate32(lw, n, T):
    """iw_reduce_kernel in numpy float32: lanes stride over k, add in order, butterfly"""
    lw = np.asarray(lw, F32)
    B, K = lw.shape
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(lw), -np.inf, lw).max(1).astype(F32)          # fmaxf drops a NaN operand
        tot = butterfly(lane_sums(lw, F32))
        shift = np.where(np.isinf(m), F32(0), m).astype(F32)
        w = np.exp(lw - shift[:, None])
        s1, s2 = butterfly(lane_sums(w, F32)), butterfly(lane_sums(w * w, F32))
        q = np.empty((B, T + 1), F32)
        for c in range(T + 1):
            q[:, c] = butterfly(lane_sums(np.where(np.asarray(n) == c, w, F32(0)), F32)) / s1
        return dict(iw_bound=shift + np.log(s1) - np.log(F32(K)), elbo=tot / F32(K), ess=s1 * s1 / s2, q_n=q)


# what the kernel's "usual logsumexp convention" comes to, per output, for one image of K = 5 particles with counts (0, 1, 2, 1, 0):
# name -> (log-weights, iw_bound, elbo, ess, q_n); "nan" stands for any NaN, a number for exactly that value
_NINF, _PINF = float("-inf"), float("inf")
RED_NONFINITE = {
    "all_ninf": ([_NINF] * 5, _NINF, _NINF, "nan", ["nan", "nan", "nan"]),
    "one_pinf": ([-3000.0, _PINF, -2990.0, -3100.0, -2950.0], _PINF, _PINF, "nan", [0.0, "nan", 0.0]),
    "one_nan": ([-3000.0, -2990.0, NAN, -3100.0, -2950.0], "nan", "nan", "nan", ["nan", "nan", "nan"]),
}
RED_NONFINITE_COUNTS = [0, 1, 2, 1, 0]


def accumulate64(iw_bound, elbo, ess, q_n, gt, acc0):
    """iw_accumulate_kernel in numpy float64, in its stated order: thread i takes images i, i + 256, ... in order; then the halving
    tree 128, 64, ... 1 over the threads; acc += the totals.  The arg-max keeps the first maximum (`>`): a tie goes to the smaller count.
    `defect` of the host test: see argmax_counts"""
    B = len(iw_bound)
    a = np.zeros((4, 256), F64)
    best = argmax_counts(q_n)
    for b in range(B):
        t = b % 256
        a[0, t] += F64(iw_bound[b]); a[1, t] += F64(elbo[b]); a[2, t] += F64(ess[b])
        if gt is not None:
            a[3, t] += 1.0 if best[b] == gt[b] else 0.0
    half = 128
    while half > 0:
        a[:, :half] = a[:, :half] + a[:, half:2 * half]
        half >>= 1
    acc = np.array(acc0, F64).copy()
    acc[:4] += a[:, 0]
    acc[4] += float(B)
    return acc


def argmax_counts(q_n, tie_to_larger=False):
    q = np.asarray(q_n)
    if tie_to_larger:
        return q.shape[1] - 1 - np.argmax(q[:, ::-1], 1)
    best = np.zeros(len(q), np.int64)
    qb = q[:, 0].copy()
    for c in range(1, q.shape[1]):
        take = q[:, c] > qb
        best, qb = np.where(take, c, best), np.where(take, q[:, c], qb)
    return best


# ---------------------------------------------------------------------------------------------------------------
# Pp: air_particle_spread (float64 in the kernel: the bound is one float32 rounding of the result + a float64 term)
# ---------------------------------------------------------------------------------------------------------------
SPREAD_CASES = {f"Spr_K{K}_B{B}_T{T}": dict(K=K, B=B, T=T) for K, B, T in
                [(1, 1, 1), (5, 5, 3), (64, 5, 3), (65, 5, 32), (200, 5, 3), (200, 1, 32), (65, 1, 1)]}


@functools.lru_cache(maxsize=None)
def spread_data(name):
    """-> logw [B, K], n [B, K], where [T, B * K, 4]; images by b % 5: 0 weights over 1000 nats, 1 a step nobody has and a step one
    particle has, 2 `where` = 1e4 + 1e-3 noise (the two-pass form), 3 single -inf weights, 4 plain"""
    c = SPREAD_CASES[name]
    K, B, T = c["K"], c["B"], c["T"]
    rng = np.random.default_rng(_seed(name))
    lw = (-3000.0 + rng.uniform(-2.0, 2.0, (B, K))).astype(F32)
    n = rng.integers(0, T + 1, (B, K)).astype(np.int32)
    where = rng.standard_normal((T, B, K, 4)).astype(F32)
    planted = {}
    for b in range(B):
        kind = b % 5
        if kind == 0 and K > 1:
            lw[b] = (-3000.0 + rng.uniform(-500.0, 500.0, K)).astype(F32)
        elif kind == 1 and T >= 3 and K >= 5:
            n[b] = np.minimum(n[b], T - 2)                                   # step T - 1 has no particle,
            lone = K - 2                                                     # step T - 2 exactly one -- and not the heaviest
            lw[b, lone] = lw[b].max() - F32(1.75)
            n[b, lone] = T - 1
            planted[b] = dict(empty=T - 1, single=T - 2, lone=lone)
        elif kind == 2:
            where[:, b] = (1e4 + 1e-3 * rng.standard_normal((T, K, 4))).astype(F32)
        elif kind == 3 and K >= 5:
            lw[b, 1::4] = -np.inf
    return dict(logw=lw, n=n, where=np.ascontiguousarray(where.reshape(T, B * K, 4)), planted=planted)


def spread_ref64(lw, n, where, T, defect=None, lanes=False):
    """numpy float64 -> mean [T, B, 4], std [T, B, 4], presence_iw [T, B] and the S of the float64 term; lanes: the sums in the
    kernel's lane order (the restatement the float64 term is measured on) instead of numpy's"""
    lw64 = np.asarray(lw, F64)
    B, K = lw64.shape
    x = np.asarray(where, F64).reshape(T, B, K, 4)

    def total(v):                                                            # over the particle axis (last)
        return butterfly(lane_sums(v, F64)) if lanes else v.sum(-1)

    with np.errstate(all="ignore"):
        w = np.exp(lw64 - lw64.max(1, keepdims=True))
        tot = total(w)
        mean, std, pres, S_mean = (np.empty((T, B, 4)), np.empty((T, B, 4)), np.empty((T, B)), np.empty((T, B, 4)))
        for t in range(T):
            has = (np.asarray(n) >= t) if defect == "has_step_ge" else (np.asarray(n) > t)
            wt = np.where(has, w, 0.0)
            W = total(wt)
            cnt = (wt > 0).sum(-1)                                           # one particle of non-zero weight: the spread is exactly 0
            if defect == "no_single_rule":
                cnt = np.zeros_like(cnt)
            for j in range(4):
                mean[t, :, j] = total(wt * x[t, :, :, j]) / W
                d = x[t, :, :, j] - mean[t, :, j][:, None]
                q = total(wt * (d * d)) / W
                std[t, :, j] = np.where((cnt == 1) & ~np.isnan(q), 0.0, np.sqrt(np.where(q < 0, 0.0, q)))
                S_mean[t, :, j] = (wt * np.abs(x[t, :, :, j])).sum(-1) / W
            pres[t] = W / tot
    D = depth(K) + 4.0
    return dict(mean=mean, std=std, presence_iw=pres, S_mean=D * S_mean, S_std=D * std + D * S_mean, S_presence_iw=D * pres)


def spread_bound(ref, S):
    """one float32 rounding of the result (+ TINY where it is not 0: a share of 1e-50 is 0 in float32) + the float64 term"""
    ref = np.asarray(ref, F64)
    return U * np.abs(ref) + np.where(ref != 0, TINY, 0.0) + SPREAD_F64_CONST * 2.0 ** -53 * np.asarray(S)


# ---------------------------------------------------------------------------------------------------------------
# Pp: air_particle_select (every output exact: the float64 sum of the two float32 values decides)
# ---------------------------------------------------------------------------------------------------------------
def select_ref(log_w, log_q, n, criterion):
    """-> best_particle, best_score (float32; NaN: the bits 0x7fc00000), num_objects, degenerate, per image"""
    B, K = log_w.shape
    with np.errstate(all="ignore"):
        s = np.asarray(log_w, F64) + (np.asarray(log_q, F64) if criterion == 1 else 0.0)
    best, score, num, deg = np.zeros(B, np.int32), np.zeros(B, F32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        ok = ~np.isnan(s[b])
        if ok.any():
            k = int(np.flatnonzero(ok & (s[b] == s[b][ok].max()))[0])       # the smallest k attaining the maximum; +-inf are values
            best[b], score[b] = k, F32(s[b, k])
        else:
            best[b], deg[b] = 0, 1
            score[b] = np.array([QNAN_BITS], np.uint32).view(F32)[0]
        num[b] = n[b, best[b]]
    return best, score, num, deg


# ---------------------------------------------------------------------------------------------------------------
# Gn: air_prior_latents, air_observe
# ---------------------------------------------------------------------------------------------------------------
GEN_PRIORS = (0.3, 1.5, 0.6, 0.4, -0.2, 0.7)
GEN_GUARD = 1e-3
GEN_ROWS = {
    "Gn_32x5x8": dict(T=32, R=5, A=8, off={}),
    "Gn_3x7x50": dict(T=3, R=7, A=50, off={}),
    "Gn_1x1x1": dict(T=1, R=1, A=1, off={}),
    "Gn_2x257x6": dict(T=2, R=257, A=6, off={}),
    "Gn_3x5x52": dict(T=3, R=5, A=52, off={}),
}
for _name in ("eps_what", "what"):
    for _o in (1, 2):
        GEN_ROWS[f"Gn_3x5x52_{_name}_{4 * _o}B"] = dict(T=3, R=5, A=52, off={_name: _o}, data="Gn_3x5x52")
for _o in (1, 2):
    GEN_ROWS[f"Gn_3x5x52_all_{4 * _o}B"] = dict(T=3, R=5, A=52, off={"eps_what": _o, "what": _o}, data="Gn_3x5x52")
for _c in GEN_ROWS.values():
    _c["V"] = iw_vec(_c["A"], _c["off"])
GEN_BIT_PEERS = {1: "Gn_3x5x52_all_4B", 2: "Gn_3x5x52_all_8B"}
DYADIC_TABLE = [0.25, 0.25, 0.5, 0.0]                                      # T = 3; u * total is exact
DYADIC_U = [0.0, 0.25, 0.5, float(np.nextafter(F32(1), F32(0))), 0.125, 0.75]
DYADIC_N = [0, 1, 2, 2, 0, 2]                                              # cum = .25, .5, 1.0 (c < T = 3); `cum <= thresh` counts a boundary


@functools.lru_cache(maxsize=None)
def gen_data(name):
    c = GEN_ROWS[name]
    if c.get("data"):
        return gen_data(c["data"])
    T, R, A = c["T"], c["R"], c["A"]
    rng = np.random.default_rng(_seed(name))
    table = rng.uniform(0.05, 1.0, T + 1)
    if T >= 3:
        table[1] = 0.0                                                       # a weight of exactly zero is stepped over
    eps_where = rng.standard_normal((T, R, 4)).astype(F32)
    if R >= 5:                                                               # the guard: scale components inside +-guard come out at +-guard
        loc, sc = F32(GEN_PRIORS[2]), F32(GEN_PRIORS[3])
        eps_where[0, 1, 0] = (F32(2e-4) - loc) / sc
        eps_where[0, 2, 2] = (F32(-3e-4) - loc) / sc
        eps_where[0, 3, 1] = (F32(2e-4) - F32(GEN_PRIORS[4])) / F32(GEN_PRIORS[5])   # a shift component: left alone
    return dict(table=table, u=rng.uniform(0.0, 1.0, R).astype(F32), eps_what=rng.standard_normal((T, R, A)).astype(F32),
                eps_where=eps_where, n_in=rng.integers(-3, T + 4, R).astype(np.int32))


def count_by_inversion(table, u, T, strict=False):
    """n = #{c < T : cum_c <= u * total} in float64, in the kernel's index order; strict: the planted defect `cum < thresh`"""
    out = []
    for ur in np.asarray(u, F32):
        total = 0.0
        for c in range(T + 1):
            total += float(table[c])
        thresh, cum, n = float(ur) * total, 0.0, 0
        for c in range(T):
            cum += float(table[c])
            n += int(cum < thresh if strict else cum <= thresh)
        out.append(n)
    return np.array(out, np.int32)


def latents_ref64(d, T, guard, n):
    """-> what64, where64, presence, S_what, S_where (|loc| + |scale * eps|); the guard acts on the float64 value like the kernel's on its own"""
    pw_loc, pw_scale, ps_loc, ps_scale, ph_loc, ph_scale = (float(F32(v)) for v in GEN_PRIORS)
    e = d["eps_where"].astype(F64)
    even = (np.arange(4) % 2 == 0)[None, None, :]
    loc, sc = np.where(even, ps_loc, ph_loc), np.where(even, ps_scale, ph_scale)
    where = loc + sc * e
    g = float(F32(guard))
    guarded = even & (np.abs(where) < g) & (g > 0)
    where = np.where(guarded, np.copysign(g, where), where)
    what = pw_loc + pw_scale * d["eps_what"].astype(F64)
    pres = (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(F32)
    return dict(what=what, where=where, presence=pres, S_what=abs(pw_loc) + np.abs(pw_scale * d["eps_what"].astype(F64)),
                S_where=np.abs(loc) + np.abs(sc * e), guarded=guarded)


def latents_restate32(d):
    pr = [F32(v) for v in GEN_PRIORS]
    e = d["eps_where"]
    even = (np.arange(4) % 2 == 0)[None, None, :]
    where = np.where(even, pr[2] + pr[3] * e, pr[4] + pr[5] * e).astype(F32)
    return (pr[0] + pr[1] * d["eps_what"]).astype(F32), where


OBS_N = (1, 3, 4, 5, 4 * 625 + 3)                                          # 626 quads: three workgroups, the last quad incomplete
OBS_SEED = 0x2545F4914F6CDD1D
OBS_OFFSET = 1000


def observe_ref(canvas, mult, std, counter_base, lo, hi, noise=True):
    """-> mean32 (the bits of mult * canvas), obs64, bound: group J's bar on the normal times std, two float32 roundings of the sum,
    and the clamp (1-Lipschitz; a NaN bound clamps nothing; a NaN pixel under a finite `lo` comes out as `lo`: fmaxf drops the NaN)"""
    canvas = np.asarray(canvas, F32)
    n = len(canvas)
    mean = (F32(mult) * canvas).astype(F32)
    m64 = mean.astype(F64)
    if noise:
        z = FC.noise_ref(OBS_SEED, OBS_OFFSET + counter_base, n, 0)[0].numpy()
        obs = m64 + float(F32(std)) * z
        bnd = float(F32(std)) * FC.NORMAL_TOL[0] * (np.abs(z) + 1.0) + 2.0 * U * (np.abs(m64) + np.abs(float(F32(std)) * z))
    else:
        obs, bnd = m64.copy(), np.zeros(n)
    if not np.isnan(lo):
        obs = np.where(np.isnan(obs), lo, np.maximum(obs, lo))
    if not np.isnan(hi):
        obs = np.where(np.isnan(obs), hi, np.minimum(obs, hi))
    return mean, obs, bnd


def observe_form(off, std, obs_given):
    """the launch rule of air_observe: off = the float offsets of canvas / mean_out / obs_out (None: NULL)"""
    vec = all(o is None or (4 * o) & 15 == 0 for o in off)
    noise = std != 0.0 and obs_given
    return "observe_kernel<%s, %s>" % ("true" if vec else "false", "true" if noise else "false")


# (offsets, std, obs_out given) of the launches tests/test_readout_kernels.py makes: every instantiation of observe_kernel
OBS_FORMS = [((0, 0, 0), 0.3, True), ((0, 0, 0), 0.0, True), ((1, 0, 0), 0.3, True), ((0, 1, 0), 0.0, True), ((0, 0, 1), 0.3, True),
             ((0, 0, None), 0.3, False), ((0, None, 0), 0.3, True)]


# ---------------------------------------------------------------------------------------------------------------
# Ps: air_parse_objects (parse_count_kernel, parse_scan_kernel, parse_scatter_kernel<V>)
# ---------------------------------------------------------------------------------------------------------------
PS_H, PS_W = 21, 19
PS_ROWS = {
    "Ps_1x1x1": dict(T=1, R=1, A=1, off={}),
    "Ps_3x5x6": dict(T=3, R=5, A=6, off={}),
    "Ps_3x5x5": dict(T=3, R=5, A=5, off={}),
    "Ps_3x9x8": dict(T=3, R=9, A=8, off={}),
    "Ps_3x9x8_what_4B": dict(T=3, R=9, A=8, off={"what": 1}),
    "Ps_3x9x8_obj_what_8B": dict(T=3, R=9, A=8, off={"obj_what": 2}),
    "Ps_32x9x4": dict(T=32, R=9, A=4, off={}),
    "Ps_32x5x2": dict(T=32, R=5, A=2, off={}),
}
for _c in PS_ROWS.values():
    _c["V"] = iw_vec(_c["A"], _c["off"])
PS_SCAN_R = (1, 1023, 1024, 1025, 2049)
PS_BOX_CONST = 4.0                 # left = ((1 - s) + t) * W / 2: three float32 roundings (the halving is exact) of values no larger than 2 S, S = W (1 + |s| + |t|) / 2; width = W s: one


@functools.lru_cache(maxsize=None)
def ps_data(name):
    """presence_prob [T, R] with the planted rows (R >= 5, T >= 3): 0 (0.5, 0, ...): m_0 == m_1; 1 all 0.5; 2 all exactly 1; 3 all exactly
    0; 4 a NaN at step 1; `where` row (0, 0) has a negative and a zero scale"""
    c = PS_ROWS[name]
    T, R, A = c["T"], c["R"], c["A"]
    rng = np.random.default_rng(_seed(name[:8]))
    prob = rng.uniform(0.02, 0.98, (T, R)).astype(F32)
    if R >= 5 and T >= 3:
        prob[:, 0] = 0.0
        prob[0, 0] = 0.5
        prob[:, 1], prob[:, 2], prob[:, 3] = 0.5, 1.0, 0.0
        prob[0, 4], prob[1, 4] = 0.9, NAN
    where = rng.uniform(-1.0, 1.0, (T, R, 4)).astype(F32)
    where[0, 0] = [-0.5, 0.2, 0.0, -0.3]
    return dict(prob=prob, where=where, what=rng.standard_normal((T, R, A)).astype(F32),
                n_in=rng.integers(-2, T + 3, R).astype(np.int32))


def count_chain64(prob):
    """parse_count_kernel's float64 chain in its index order -> n^ [R] (the smallest n attaining the maximum; a NaN term never wins),
    q64 [R, T + 1] = m / sum m, score64 [T, R] = sum_{n > t} q(n)"""
    p = np.asarray(prob, F32).astype(F64)
    T, R = p.shape
    cum, S, best, n_hat, m_all = np.ones(R), np.zeros(R), np.zeros(R), np.zeros(R, np.int32), np.empty((R, T + 1))
    with np.errstate(all="ignore"):
        for n in range(T + 1):
            m = (1.0 - p[n]) * cum if n < T else cum.copy()
            if n < T:
                cum = cum * p[n]
            S = S + m
            take = (m > best) if n else np.ones(R, bool)
            best, n_hat = np.where(take, m, best), np.where(take, n, n_hat).astype(np.int32)
            m_all[:, n] = m
        q = m_all / S[:, None]
        score = np.stack([q[:, t + 1:].sum(1) for t in range(T)])
    return n_hat, q, score


def boxes64(where, H, W):
    """evaluation.attention_box in float64, row by row -> boxes [.., 4] and the S of each component"""
    from attend_infer_repeat_amd.evaluation import attention_box
    w = np.asarray(where, F32).astype(F64)
    flat = w.reshape(-1, 4)
    box = np.array([attention_box(row, W, H) for row in flat]).reshape(w.shape)
    sx, tx, sy, ty = (np.abs(w[..., k]) for k in range(4))
    S = np.stack([W * (1 + sx + tx) / 2, H * (1 + sy + ty) / 2, W * sx, H * sy], -1)
    return box, S


def exclusive_scan(counts, carry=True):
    """offsets [R + 1]; carry = False: the planted defect -- the base not carried across the passes of 1024"""
    counts = np.asarray(counts, np.int64)
    out = np.zeros(len(counts) + 1, np.int64)
    out[1:] = np.cumsum(counts)
    if not carry:
        for r0 in range(1024, len(counts), 1024):
            out[r0:r0 + 1024] -= out[r0]
        out[-1] = counts[(len(counts) - 1) // 1024 * 1024:].sum() if len(counts) else 0
    return out.astype(np.int32)


def object_table(n, offsets, score, boxes, where, what):
    """the flat table (image-major, step order inside an image) from the launch's own per-step outputs -> dict of arrays with
    offsets[R] rows"""
    T, R = score.shape
    rows = [(r, t) for r in range(R) for t in range(int(n[r]))]
    assert [int(offsets[r]) + t for r, t in rows] == list(range(len(rows)))
    ri, ti = np.array([r for r, _ in rows], np.int64), np.array([t for _, t in rows], np.int64)
    return dict(obj_image=ri.astype(np.int32), obj_step=ti.astype(np.int32), obj_score=score[ti, ri], obj_box=boxes[ti, ri],
                obj_where=where[ti, ri], obj_what=what[ti, ri])


# ---------------------------------------------------------------------------------------------------------------
# Ps: air_parse_render
# ---------------------------------------------------------------------------------------------------------------
PR_MULT, PR_STD = 0.75, 0.3
PR_NREF = 6                        # images with a CPU reference; the others repeat them (b % PR_NREF) and must repeat their bits
PARSE_TAIL_FLOATS, CV_MAX_LDS, ST_THREADS = 2 * 32 + 32, 160 * 1024, 256


def render_form(T, R, H, W, h, w, n_bands, glimpse_off=0):
    """Python mirror of the form rule of air_parse_render (held against air_parse_render_form by the host test) + `rule`, the thread
    rule taken: "px" (one pixel per thread, at most 1024), "512", "st" (ST_THREADS)"""
    nb = max(1, min(n_bands, H))
    rb = -(-H // nb)
    nb = -(-H // rb)
    lds = 4 * (T * (((h + 2) * (w + 2) + 3) & ~3) + 2 * T * (W + rb) + PARSE_TAIL_FLOATS)
    units = R * nb
    threads, rule = (512, "512") if units <= 512 else (ST_THREADS, "st")
    if units <= 256:
        px = rb * W
        threads, rule = (1024 if px >= 1024 else ((px + 63) // 64) * 64), "px"
    return dict(kernel=6, NB=nb, RB=rb, threads=threads, lds_bytes=lds, vec4_glimpse=int(w % 4 == 0 and (4 * glimpse_off) % 16 == 0),
                items=units, fixed_cap=2048, resident_cap=int(units > 2048), rule=rule)


def _pr(H, W, h, w, T, R, bands, reaches, **kw):
    return dict(H=H, W=W, h=h, w=w, T=T, R=R, bands=bands, reaches=reaches, off=kw.pop("off", {}), **kw)


PR_ROWS = {
    "Pr_21x19_odd_W": _pr(21, 19, 6, 10, 3, 2, 1, "odd W: pack_ok false for odd b; 399 pixels, the px thread rule", planted=True),
    "Pr_8x16": _pr(8, 16, 4, 4, 2, 3, 1, "pack_ok true, vec4_glimpse true", presence="101_and_absent"),
    "Pr_8x16_2bands": _pr(8, 16, 4, 4, 2, 3, 2, "two bands"),
    "Pr_8x16_owner_1B": _pr(8, 16, 4, 4, 2, 3, 2, "owner 1 byte off: bytes, never packed", off={"owner": 1}, data="Pr_8x16_2bands"),
    "Pr_8x16_glimpse_4B": _pr(8, 16, 4, 4, 2, 3, 2, "glimpse 4 bytes off: the scalar staging", off={"glimpse": 1}, data="Pr_8x16_2bands"),
    "Pr_5x6": _pr(5, 6, 3, 3, 3, 2, 1, "npx = 30: the last quad is cut by npx", presence="101_and_absent", twins=True),
    "Pr_65x64": _pr(65, 64, 5, 7, 2, 1, 1, "4160 pixels on 1024 threads: the second prefetch", presence="all"),
    "Pr_R300": _pr(6, 10, 3, 3, 2, 300, 1, "512 threads"),
    "Pr_R600": _pr(6, 10, 3, 3, 2, 600, 1, "ST_THREADS"),
    "Pr_R2049": _pr(6, 10, 3, 3, 2, 2049, 1, "capped grid: a workgroup renders a second unit into the same carve"),
    "Pr_T32": _pr(8, 8, 3, 3, 32, 2, 1, "bit 31 of pmask", presence="all"),
    "Pr_nan_glimpse": _pr(8, 16, 4, 4, 3, 2, 1, "a NaN in one glimpse", nan_glimpse=True, presence="all"),
}


def pr_pack_ok(name):
    """the values pack_ok takes over the row's units"""
    c = PR_ROWS[name]
    f = render_form(c["T"], c["R"], c["H"], c["W"], c["h"], c["w"], c["bands"])
    al = c["off"].get("owner", 0) % 4 == 0
    return {bool(al and (b * c["H"] * c["W"] + band * f["RB"] * c["W"]) % 4 == 0) for b in range(min(c["R"], 8)) for band in range(f["NB"])}


@functools.lru_cache(maxsize=None)
def pr_data(name):
    c = PR_ROWS[name]
    if c.get("data"):
        return pr_data(c["data"])
    T, R, H, W, h, w = (c[k] for k in ("T", "R", "H", "W", "h", "w"))
    nref = min(R, PR_NREF)
    rng = np.random.default_rng(_seed(name))
    glm = rng.uniform(0.05, 1.0, (T, nref, h, w)).astype(F32)
    where = WC.draw_where(T * nref, "write", H, W, h, w, rng).reshape(T, nref, 4)
    if c.get("planted"):
        rows = list(WC.planted_rows("write", H, W, h, w).values())
        for i, row in enumerate(rows[:T * nref - 1]):
            where.reshape(-1, 4)[i + 1] = row
    kind = c.get("presence", "random")
    pres = (rng.uniform(size=(T, nref)) < 0.7).astype(F32)
    if kind == "all":
        pres[:] = 1.0
    elif kind == "101_and_absent":
        pres[:, 0] = (np.arange(T) % 2 == 0)                                 # a non-monotone row: the render takes presences as given
        pres[:, 1] = 0.0                                                     # all absent: canvas exactly 0, owner -1 everywhere
    if c.get("twins"):                                                       # two steps with identical glimpse and where: the smaller owns
        glm[2, 0], where[2, 0], pres[0, 0], pres[2, 0] = glm[0, 0], where[0, 0], 1.0, 1.0
    if c.get("nan_glimpse"):
        glm[1, 0, h // 2, w // 2] = NAN
    obs = rng.uniform(0.0, 1.0, (nref, H, W)).astype(F32)
    rep = np.arange(R) % nref
    return dict(glimpse=glm[:, rep], where=np.ascontiguousarray(where[:, rep]), presence=pres[:, rep], obs=obs[rep], nref=nref)


@functools.lru_cache(maxsize=None)
def pr_ref64(name):
    """float64 through warp_cases.warp64 -> layers [T, nref, H, W] (absent: 0), reconstruction, their S (group X's), the per-pixel
    reconstruction term and its S"""
    c, d = PR_ROWS[name], pr_data(name)
    T, H, W, h, w, nref = c["T"], c["H"], c["W"], c["h"], c["w"], d["nref"]
    K = T * nref
    wh = d["where"][:, :nref].reshape(K, 4)
    ax, bx = WC.axis_ab(wh, "write", 0)
    ay, by = WC.axis_ab(wh, "write", 1)
    g = d["glimpse"][:, :nref].reshape(K, h, w).astype(F64)
    hole = np.isnan(g)                                                       # a NaN cell reaches the pixels whose four taps include it
    fw = WC.warp64(np.where(hole, 0.0, g), ax, bx, ay, by, W, H, np.zeros((K, H, W)))
    if hole.any():
        reach = WC.warp64(hole.astype(F64), ax, bx, ay, by, W, H, np.zeros((K, H, W)))["out"] > 0    # (no coordinate is an integer: weights > 0)
        fw["out"] = np.where(reach, NAN, fw["out"])
    mult, std = float(F32(PR_MULT)), float(F32(PR_STD))
    p = (d["presence"][:, :nref] > 0.5).astype(F64)[:, :, None, None]
    v, vabs = fw["out"].reshape(T, nref, H, W), fw["S_out_coord"].reshape(T, nref, H, W)
    layers, S_layers = mult * np.where(p > 0, v, 0.0), mult * np.where(p > 0, vabs, 0.0)
    rec, S_rec = layers.sum(0), S_layers.sum(0)
    S_layers, S_rec = np.where(np.isnan(layers), 0.0, S_layers), np.where(np.isnan(rec), 0.0, S_rec)
    z = (d["obs"][:nref].astype(F64) - rec) / std
    cst = 0.5 * np.log(2 * np.pi) + np.log(std)
    return dict(layers=layers, S_layers=S_layers, reconstruction=rec, S_reconstruction=S_rec, rec_pix=0.5 * z * z + cst,
                S_rec_pix=z * z + np.abs(z) * (np.abs(d["obs"][:nref]) + S_rec) / std + abs(cst))


def owner_rule(layers, presence, thr, tie_to_larger=False, ge=False):
    """owner [R, H, W] int8 from layers [T, R, H, W] (float32, the launch's own): the smallest present t attaining the maximum (a NaN
    never does), -1 unless that maximum is > thr; the two planted defects: the tie to the larger step, `top >= thr`"""
    T, R = presence.shape
    top = np.full(layers.shape[1:], -np.inf, F32)
    own = np.full(layers.shape[1:], -1, np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            take = ((layers[t] >= top) if tie_to_larger else (layers[t] > top)) & (presence[t] > 0.5)[:, None, None]
            top, own = np.where(take, layers[t], top), np.where(take, t, own).astype(np.int8)
        keep = (top >= F32(thr)) if ge else (top > F32(thr))
    return np.where(keep, own, -1).astype(np.int8), top


# ---------------------------------------------------------------------------------------------------------------
# coverage: the kernels of the four files, and the rows that name them
# ---------------------------------------------------------------------------------------------------------------
INSTANTIATIONS = ("iw_logweight_kernel<4>", "iw_logweight_kernel<2>", "iw_logweight_kernel<1>", "iw_logposterior_kernel<4>",
                  "iw_logposterior_kernel<2>", "iw_logposterior_kernel<1>", "iw_reduce_kernel", "iw_accumulate_kernel",
                  "particle_argmax_kernel", "particle_gather_kernel", "particle_spread_kernel", "prior_latents_kernel<4>",
                  "prior_latents_kernel<2>", "prior_latents_kernel<1>", "observe_kernel<true, true>", "observe_kernel<true, false>",
                  "observe_kernel<false, true>", "observe_kernel<false, false>", "parse_count_kernel", "parse_scan_kernel",
                  "parse_scatter_kernel<4>", "parse_scatter_kernel<2>", "parse_scatter_kernel<1>", "parse_render_kernel")


def named_instantiations():
    names = set()
    for c in IW_ROWS.values():
        names |= {f"iw_logweight_kernel<{c['V']}>", f"iw_logposterior_kernel<{c['V']}>"}
    for c in GEN_ROWS.values():
        names.add(f"prior_latents_kernel<{c['V']}>")
    for off, std, given in OBS_FORMS:
        names.add(observe_form(off, std, given))
    for c in PS_ROWS.values():
        names |= {"parse_count_kernel", f"parse_scatter_kernel<{c['V']}>"}
    if RED_CASES:
        names |= {"iw_reduce_kernel", "iw_accumulate_kernel"}
    if SPREAD_CASES:
        names |= {"particle_spread_kernel", "particle_argmax_kernel", "particle_gather_kernel"}
    if max(PS_SCAN_R) > 1024:
        names.add("parse_scan_kernel")
    if PR_ROWS:
        names.add("parse_render_kernel")
    return names
