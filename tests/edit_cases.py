"""Cases, float64 references, numpy float32 restatements (one rounding per operation), bounds and planted defects for the kernel-level
tests of the three stages that edit a parse: groups Rf (air_refine_step), Pn (air_prune_score, air_prune_select) and Pr
(air_propose_residual, air_propose_pool, air_propose_source).  tests/test_edit_kernels.py runs them on the device one launch at a time,
tests/test_edit_cases_host.py holds this module on the CPU.  Windows, sentinels, the lane sums and the bound helpers come from
tests/readout_cases.py, the transforms and the float64 warp from tests/warp_cases.py.

Bounds are elementwise, CONST * 2^-24 * S; every CONST is four times the worst ratio of the float32 restatement of the kernel's own
order, rounded up (RESTATEMENT_SHARE = 0.25); the measured ratios are in RESTATEMENT_RATIO and DESIGN.md.

Rf.  J: S = depth(n A / V) * sum(z^2 / 2 + |log scale| + log(2 pi) / 2 over the counted items) + |rec|; rec is the float32 band-order
sum (exact in the closing float64 add).  The update, per element: g = d + (z - mu) / var, S_g = |d| + |z - mu| / var;
m' = b1 m + (1 - b1) g, S_m = |b1 m| + (1 - b1) S_g;  v' = b2 v + (1 - b2) g^2, S_v = |b2 v| + (1 - b2) (g^2 + 2 |g| S_g);
z' = z - step, step = lr (m' / c1) / (sqrt(v' / c2) + eps), S_z = |z| + |z'| + 6 |step| + the step's first-order change under S_m and
S_v: lr S_m / (c1 den) + |step| S_v / (2 c2 sqrt(v' / c2) den).  The refine file carries no `fp contract(off)`: the device may fuse
b1 * m + (1 - b1) * g and z - lr * q where the restatement rounds twice; a fused operation has one rounding fewer, the share absorbs it.

Pn score, per (band, image, mask), S in four parts: (1) the layers' error, group X's CONST * S_layers (warp_cases: the taps' magnitudes
plus the coordinate term), reaches the pixel's term through d(z^2 / 2) = |z| * mult / std * d(canvas);  (2) the roundings of the pixel's
own operations, z^2 + |z| (|obs| + mult S_canvas) / std + |z^2 / 2 + cst|;  (3) cst = log(2 pi) / 2 + log(std) is rounded once and
repeats in every pixel, so its error does not average out under the sum: npx * |cst|, once;  (4) the sum itself, a thread adds
ceil(npx / 256) terms, the wave's butterfly 6, the wave totals 3: that many roundings of sum |term|.

Pn select: J_sub, S = depth(A / V) * (the latent terms' magnitudes of every set step) + |rec| + |log pi|; every other output is exact,
by the rule applied to the device's own J_sub (prune.reference_select with J_sub given).

Pr residual: res is the bits of the rule on the float32 canvas of air_parse_render; against float64 the bound is RES_CONST * 2^-24 *
(|obs| + mult * S_canvas), RES_CONST = group X's CONST + 2: X's bound on the canvas, one rounding of mult * canvas and one of the
subtraction, each at most 2^-24 * S.  res_parts: the pixel errors carried through 2 r dr, the squares' own rounding and the sum."""
import functools
import zlib

import numpy as np

import readout_cases as RC
import warp_cases as WC
from readout_cases import F32, F64, U, NAN, depth, butterfly  # noqa: F401
from warp_cases import DEFECT_MARGIN, N_REF, RESTATEMENT_SHARE  # noqa: F401

HALF_LOG_2PI = 0.91893853320467274178   # (the kernels' constant is this, rounded to float32)
PAYLOAD_BITS = 0x7fa00001          # a NaN with a payload: a bit copy keeps it, arithmetic would not
CV_MAX_LDS = 160 * 1024

# the worst float32-restatement ratio (error / (2^-24 S)) per bound, measured on the CPU by
# tests/test_edit_cases_host.py::test_restatements_keep_their_share (which prints them with -s), and four times it, rounded up
RESTATEMENT_RATIO = {"rf_J": 0.192, "rf_m": 2.865, "rf_v": 1.911, "rf_z": 0.490, "sel_J": 0.248, "score": 0.134}
CONST = {k: float(np.ceil(4 * v)) for k, v in RESTATEMENT_RATIO.items()}
RES_CONST = WC.CONST["X"] + 2.0


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def vec_rule(A, what_off=0):
    """the V of refine_step_kernel<V> / prune_select_kernel<V>: from A and from where `what` starts (what_off in floats)"""
    return 4 if A % 4 == 0 and what_off % 4 == 0 else (2 if A % 2 == 0 and what_off % 2 == 0 else 1)


PRESENCE_KINDS = ("ones", "zero", "101", "half", "nan")


def presence_row(kind, T):
    """-> (row [T], n): ones; zero; (1, 0, 1, ..): one leading one; a 0.5 behind one one (T = 1: in front): absent; a NaN likewise"""
    row = np.ones(T, F32)
    if kind == "zero":
        row[:] = 0.0
    elif kind == "101":
        row[:] = np.arange(T) % 2 == 0
    elif kind in ("half", "nan"):
        row[min(1, T - 1)] = 0.5 if kind == "half" else NAN
    with np.errstate(invalid="ignore"):
        n = int(np.argmin(np.concatenate([row > 0.5, [False]])))
    return row, n


def leading_ones(presence):
    with np.errstate(invalid="ignore"):
        return np.cumprod(np.asarray(presence) > 0.5, axis=0).sum(0).astype(np.int64)


def f32_band_sum(parts):
    """`for k: rec += parts[k]` in float32 from 0 (the operations of air_sum_leading) over the leading axis"""
    rec = np.zeros(parts.shape[1:], F32)
    with np.errstate(all="ignore"):
        for k in range(parts.shape[0]):
            rec = (rec + parts[k]).astype(F32)
    return rec


def _ln64(x, loc, scale):
    with np.errstate(all="ignore"):
        z = (np.asarray(x, F64) - loc) / scale
        return -0.5 * z * z - np.log(scale) - HALF_LOG_2PI, 0.5 * z * z + np.abs(np.log(scale)) + HALF_LOG_2PI


def _ln32(x, loc, scale, log_scale):
    with np.errstate(all="ignore"):
        z = (x - loc) / scale
        return (F32(-0.5) * (z * z) - log_scale - RC.HALF_LOG_2PI).astype(F32)


def where_prior(where_loc, pr, shape):
    """-> mu, sd [.., 4] float64 of the scale / shift prior; pr[4] NaN: the shift prior is centred on where_loc"""
    mu, sd = np.empty(shape, F64), np.empty(shape, F64)
    mu[..., 0::2], sd[..., 0::2] = pr[2], pr[3]
    mu[..., 1::2] = np.asarray(where_loc, F64)[..., 1::2] if np.isnan(pr[4]) else pr[4]
    sd[..., 1::2] = pr[5]
    return mu, sd


PRIORS = {"fixed": (0.3, 1.5, 0.6, 0.4, -0.2, 0.7), "centred": (0.0, 1.0, 0.5, 0.5, NAN, 0.7)}


def priors32(kind, **over):
    pr = [float(F32(v)) for v in PRIORS[kind]]
    if "what_p_scale" in over:
        pr[1] = float(F32(over["what_p_scale"]))
    return pr


# ---------------------------------------------------------------------------------------------------------------
# Rf: air_refine_step
# ---------------------------------------------------------------------------------------------------------------
RF_ADAM = dict(lr_what=0.05, lr_where=0.01, beta1=0.9, beta2=0.999, eps=1e-8, guard=1e-3)
RF_UPDATED = ("what", "where", "m_what", "v_what", "m_where", "v_where")


def _rf(T, B, A, G, bands, prior, reaches, off=None, data=None, present=False):
    off = dict(off or {})
    return dict(T=T, B=B, A=A, G=G, bands=bands, prior=prior, reaches=reaches, off=off, data=data, present=present,
                V=vec_rule(A, off.get("what", 0)))


RF_ROWS = {
    "Rf_1x1x1x1": _rf(1, 1, 1, 1, 1, "fixed", "the smallest launch"),
    "Rf_3x5x12x16": _rf(3, 5, 12, 16, 3, "centred", "V = 4; every presence row"),
    "Rf_3x5x6x9": _rf(3, 5, 6, 9, 8, "fixed", "V = 2 by A; eight bands"),
    "Rf_3x5x7x9": _rf(3, 5, 7, 9, 1, "centred", "V = 1 by A"),
    "Rf_32x3x50x400": _rf(32, 3, 50, 400, 3, "fixed", "bit 31 of the ballot, 800 what vectors over 64 lanes, a 1600-element update "
                          "over 256 threads, 128 where threads", present=True),
    "Rf_2x300x4x4": _rf(2, 300, 4, 4, 1, "centred", "more workgroups than CUs"),
    "Rf_3x5x12x16_what_4B": _rf(3, 5, 12, 16, 3, "centred", "V = 1 by the alignment of what (first run)", {"what": 1}, "Rf_3x5x12x16"),
    "Rf_3x5x12x16_what_8B": _rf(3, 5, 12, 16, 3, "centred", "V = 2 by the alignment of what (first run)", {"what": 2}, "Rf_3x5x12x16"),
    "Rf_3x5x12x16_best_what_4B": _rf(3, 5, 12, 16, 3, "centred", "the word copy of what", {"best_what": 1}, "Rf_3x5x12x16"),
    "Rf_3x5x12x16_best_glimpse_4B": _rf(3, 5, 12, 16, 3, "centred", "the word copy of glimpse", {"best_glimpse": 1}, "Rf_3x5x12x16"),
}


@functools.lru_cache(maxsize=None)
def rf_data(name):
    """float32 inputs of a row; image b has presence kind b % 5 (present: all ones); rows behind n hold NaN in what, where, where_loc,
    both gradients and the four moments, one what element there the payload NaN and one -0.0"""
    c = RF_ROWS[name]
    if c["data"]:
        return rf_data(c["data"])
    T, B, A, G = c["T"], c["B"], c["A"], c["G"]
    rng = np.random.default_rng(_seed(name))
    pres, n = np.empty((T, B), F32), np.empty(B, np.int64)
    for b in range(B):
        pres[:, b], n[b] = presence_row("ones" if c["present"] else PRESENCE_KINDS[b % 5], T)
    nrm = lambda *s: rng.standard_normal(s).astype(F32)
    d = dict(what=F32(0.3) + F32(1.2) * nrm(T, B, A), glimpse=rng.uniform(0.0, 1.0, (T, B, G)).astype(F32),
             dwhat=F32(2.0) * nrm(T, B, A), dwhere=F32(2.0) * nrm(T, B, 4), m_what=F32(0.3) * nrm(T, B, A),
             v_what=rng.uniform(0.01, 2.0, (T, B, A)).astype(F32), m_where=F32(0.3) * nrm(T, B, 4),
             v_where=rng.uniform(0.01, 2.0, (T, B, 4)).astype(F32), rec_parts=rng.uniform(5.0, 200.0, (c["bands"], B)).astype(F32))
    where = np.stack([rng.uniform(0.3, 1.2, (T, B)), rng.uniform(-0.8, 0.8, (T, B)), rng.uniform(0.3, 1.2, (T, B)),
                      rng.uniform(-0.8, 0.8, (T, B))], -1).astype(F32)
    d["where"], d["where_loc"] = where, (where + F32(0.1) * nrm(T, B, 4)).astype(F32)
    behind = np.arange(T)[:, None] >= n[None, :]
    for k in ("what", "where", "where_loc", "dwhat", "dwhere") + RF_UPDATED[2:]:
        d[k][behind] = NAN
    for b in range(B):
        if n[b] < T:
            d["what"][T - 1, b, 0] = np.array([PAYLOAD_BITS], np.uint32).view(F32)[0]
            d["what"][T - 1, b, A - 1] = F32(-0.0)
    d.update(presence=pres, n=n)
    return d


def adam64(z, d, mu, var, m, v, lr, ad, c1, c2, defect=None):
    """the float64 rule of rf_adam on float32 operands -> dict(g, m, v, z and S_*); defects: "no_prior_term", "no_bias_correction" """
    with np.errstate(invalid="ignore"):                             # (the payload NaN behind n is a signalling one)
        z, d, m, v = (np.asarray(a, F64) for a in (z, d, m, v))
    b1, b2, eps = (float(F32(ad[k])) for k in ("beta1", "beta2", "eps"))
    lr = float(F32(lr))
    if defect == "no_bias_correction":
        c1 = c2 = 1.0
    with np.errstate(all="ignore"):
        pull = np.zeros_like(z) if defect == "no_prior_term" else (z - mu) / var
        g = d + pull
        S_g = np.abs(d) + np.abs(pull)
        m2, v2 = b1 * m + (1.0 - b1) * g, b2 * v + (1.0 - b2) * (g * g)
        S_m = np.abs(b1 * m) + (1.0 - b1) * S_g
        S_v = np.abs(b2 * v) + (1.0 - b2) * (g * g + 2.0 * np.abs(g) * S_g)
        root = np.sqrt(v2 / c2)
        den = root + eps
        step = lr * (m2 / c1) / den
        z2 = z - step
        slope_v = np.where(root > 0, np.abs(step) * S_v / (2.0 * c2 * np.where(root > 0, root, 1.0) * den), 0.0)
        S_z = np.abs(z) + np.abs(z2) + 6.0 * np.abs(step) + lr * S_m / (c1 * den) + slope_v
    return dict(g=g, m=m2, v=v2, z=z2, S_m=S_m, S_v=S_v, S_z=S_z)


def adam32(z, d, mu, sc, m, v, lr, ad, c1, c2):
    """rf_adam in numpy float32, one rounding per operation (var = sc * sc is the caller's, rounded once)"""
    b1, b2, eps, lr, c1, c2 = (F32(x) for x in (ad["beta1"], ad["beta2"], ad["eps"], lr, c1, c2))
    with np.errstate(all="ignore"):
        var = (np.asarray(sc, F32) * np.asarray(sc, F32)).astype(F32)
        g = (d + (z - mu) / var).astype(F32)
        m2 = (b1 * m + (F32(1) - b1) * g).astype(F32)
        v2 = (b2 * v + (F32(1) - b2) * (g * g)).astype(F32)
        z2 = (z - lr * (m2 / c1) / (np.sqrt(v2 / c2) + eps)).astype(F32)
    return m2, v2, z2


def bias_corrections(it, ad=RF_ADAM):
    """c1, c2 of iteration `it` as the caller forms them: 1 - beta^(it + 1), rounded to float32"""
    return float(F32(1.0 - float(F32(ad["beta1"])) ** (it + 1))), float(F32(1.0 - float(F32(ad["beta2"])) ** (it + 1)))


def guard64(z, guard):
    """the guard on the scale components (0, 2) of where [.., 4]: inside (-guard, guard) -> copysign(guard, .)"""
    z = np.array(z, F64)
    g = float(F32(guard))
    if g > 0:
        s = z[..., 0::2]
        with np.errstate(invalid="ignore"):
            z[..., 0::2] = np.where(np.abs(s) < g, np.copysign(g, s), s)
    return z


def rf_ref64(d, c, pr, it, ad=RF_ADAM, V=None, defect=None, lr_what=None, lr_where=None):
    """float64 on the float32 inputs `d` of a row `c` -> J, S_J, n and (where n counts) the update of the six buffers with their S"""
    T, B, A = d["what"].shape
    V = c["V"] if V is None else V
    n = leading_ones(d["presence"])
    mask = np.arange(T)[:, None] < n[None, :]
    mu, sd = where_prior(d["where_loc"], pr, d["where"].shape)
    lw, Sw = _ln64(d["what"], pr[0], pr[1])
    lh, Sh = _ln64(d["where"], mu, sd)
    rec = f32_band_sum(d["rec_parts"]).astype(F64)
    with np.errstate(all="ignore"):
        lat = np.where(mask, lw.sum(-1) + lh.sum(-1), 0.0).sum(0)
        S_lat = np.where(mask, Sw.sum(-1) + Sh.sum(-1), 0.0).sum(0)
        J = -rec + lat
    D = np.array([depth(int(k) * A // V) for k in n], F64)
    out = dict(J=J, S_J=np.where(n > 0, D * S_lat, 0.0) + np.abs(rec), n=n, mask=mask)
    c1, c2 = bias_corrections(it, ad)
    lrs = dict(what=ad["lr_what"] if lr_what is None else lr_what, where=ad["lr_where"] if lr_where is None else lr_where)
    for base, mu_, var in (("what", pr[0], pr[1] * pr[1]), ("where", mu, sd * sd)):
        r = adam64(d[base], d["d" + base], mu_, var, d["m_" + base], d["v_" + base], lrs[base], ad, c1, c2, defect)
        if base == "where":
            r["z_raw"], r["z"] = r["z"], guard64(r["z"], ad["guard"])
        out[base] = r
    return out


def rf_restate32(d, c, pr, it, V, ad=RF_ADAM):
    """refine_step_kernel<V> in numpy float32: J (the lane layout of iw_logposterior_kernel) and the six updated buffers"""
    T, B, A = d["what"].shape
    pr32 = [F32(v) for v in pr]
    n = leading_ones(d["presence"])
    AV = A // V
    J = np.empty(B, F64)
    centred = np.isnan(pr32[4])
    with np.errstate(all="ignore"):
        l_w, l_s, l_h = np.log(pr32[1]), np.log(pr32[3]), np.log(pr32[5])
        for b in range(B):
            k = int(n[b])
            wt = _ln32(d["what"][:k, b, :AV * V].reshape(-1), pr32[0], pr32[1], l_w)
            x = d["where"][:k, b]
            locs = np.stack([np.full(k, pr32[2], F32), d["where_loc"][:k, b, 1] if centred else np.full(k, pr32[4], F32),
                             np.full(k, pr32[2], F32), d["where_loc"][:k, b, 3] if centred else np.full(k, pr32[4], F32)], 1)
            ht = _ln32(x, locs, np.array([pr32[3], pr32[5], pr32[3], pr32[5]], F32)[None], np.array([l_s, l_h, l_s, l_h], F32)[None])
            s = RC._row_sum32(wt, ht, k, AV, V)
            J[b] = -float(f32_band_sum(d["rec_parts"])[b]) + float(s)
    c1, c2 = bias_corrections(it, ad)
    mu, sd = where_prior(d["where_loc"], pr, d["where"].shape)
    out = dict(J=J)
    out["m_what"], out["v_what"], out["what"] = adam32(d["what"], d["dwhat"], pr32[0], pr32[1], d["m_what"], d["v_what"], ad["lr_what"], ad, c1, c2)
    out["m_where"], out["v_where"], out["where"] = adam32(d["where"], d["dwhere"], mu.astype(F32), sd.astype(F32), d["m_where"], d["v_where"],
                                                         ad["lr_where"], ad, c1, c2)
    return out


def keep_rule(J, best, it, defect=None):
    """take [B]: iteration 0 takes whatever J is; later a non-NaN J that is larger than the best, or any non-NaN J over a NaN best.
    Defects: "ge" (J == best taken), "nan_best_stays" (a NaN best never replaced)"""
    J, best = np.asarray(J, F64), np.asarray(best, F64)
    if it == 0:
        return np.ones(J.shape, bool)
    with np.errstate(invalid="ignore"):
        better = (J >= best) if defect == "ge" else (J > best)
        over_nan = np.zeros(J.shape, bool) if defect == "nan_best_stays" else np.isnan(best)
        return ~np.isnan(J) & (over_nan | better)


# the planted images of the edge launch (T = 1, A = 4, fixed prior): name -> image
RF_EDGE_IMAGES = {"zero_gradient": 0, "lands_inside": 1, "plain": 2}


@functools.lru_cache(maxsize=None)
def rf_edge_data():
    """T = 1, B = 3, A = 4, G = 1, every step present, m = v = 0 throughout (iteration 0).  Image 0: g is exactly 0 in every element
    (d = -((z - mu) / var) in float32), where = (guard, 2e-4, -0.0, -2e-4): the latent keeps its bits, the scale on +guard is left alone,
    -0.0 becomes -guard, the shift inside is left alone; with eps = 0 every element is 0 / 0.  Image 1: the scale components start at
    +-(lr_where + 2e-4) with a gradient of their own sign, so they land 2e-4 inside the guard on either side; its shift component 1
    starts at lr_where + 2e-4 and lands inside too: left alone.  Image 2: plain."""
    rng = np.random.default_rng(_seed("rf_edges"))
    T, B, A, G = 1, 3, 4, 1
    pr = [F32(v) for v in PRIORS["fixed"]]
    gd, lr = F32(RF_ADAM["guard"]), F32(RF_ADAM["lr_where"])
    d = dict(what=(F32(0.3) + rng.standard_normal((T, B, A))).astype(F32), glimpse=rng.uniform(0, 1, (T, B, G)).astype(F32),
             dwhat=rng.standard_normal((T, B, A)).astype(F32), dwhere=rng.standard_normal((T, B, 4)).astype(F32),
             rec_parts=rng.uniform(5.0, 50.0, (1, B)).astype(F32), presence=np.ones((T, B), F32))
    where = np.stack([rng.uniform(0.3, 1.2, (T, B)), rng.uniform(-0.8, 0.8, (T, B))] * 2, -1).astype(F32)
    where[0, 0] = [gd, F32(2e-4), F32(-0.0), F32(-2e-4)]
    where[0, 1] = [lr + F32(2e-4), lr + F32(2e-4), -(lr + F32(2e-4)), F32(0.3)]
    d["where"], d["where_loc"] = where, where.copy()
    d["dwhere"][0, 1] = [5.0, 5.0, -5.0, 1.0]
    mu = np.array([pr[2], pr[4], pr[2], pr[4]], F32)
    sc = np.array([pr[3], pr[5], pr[3], pr[5]], F32)
    d["dwhat"][0, 0] = -((d["what"][0, 0] - pr[0]) / (pr[1] * pr[1]).astype(F32))
    d["dwhere"][0, 0] = -((where[0, 0] - mu) / (sc * sc).astype(F32))
    for k in ("m_what", "v_what"):
        d[k] = np.zeros((T, B, A), F32)
    for k in ("m_where", "v_where"):
        d[k] = np.zeros((T, B, 4), F32)
    d["n"] = np.full(B, T, np.int64)
    return d


RF_EDGE_ROW = dict(T=1, B=3, A=4, G=1, bands=1, prior="fixed", off={}, V=4)

RF_REFUSALS = (
    [(k, {k: None}, -1) for k in ("what", "where", "glimpse", "presence", "rec_parts", "best_J", "best_iter", "best_what", "best_where",
                                  "best_glimpse")]
    + [(k + " under do_update", {k: None}, -1) for k in ("dwhat", "dwhere", "m_what", "v_what", "m_where", "v_where")]
    + [("where_loc under a NaN shift loc", {"where_loc": None, "prior": "centred"}, -1)]
    + [(f"{k}={v}", {k: v}, -2) for k, v in (("T", 0), ("T", 33), ("B", 0), ("A", 0), ("G", 0), ("bands", 0), ("iter", -1))]
    + [(k + "+4", {"bytes": (k, 4)}, -3) for k in ("where", "best_where", "where_loc", "dwhere", "m_where", "v_where")]
    + [("what+2", {"bytes": ("what", 2)}, -3), ("best_J+4", {"bytes": ("best_J", 4)}, -3)])


# ---------------------------------------------------------------------------------------------------------------
# the band geometry of air_prune_score / air_propose_residual, mirrored
# ---------------------------------------------------------------------------------------------------------------
def unroll_bands(R, H):
    """air_canvas_unroll_bands(R, H) -> (NB, RB)"""
    nb = min(8, 256 // max(R, 1))
    nb = max(1, min(nb, H))
    rb = -(-H // nb)
    return -(-H // rb), rb


def band_carve_floats(T, RB, W, h, w):
    return T * (((h + 2) * (w + 2) + 3) & ~3) + 2 * T * (W + RB)


def score_lds_bytes(T, RB, W, h, w):
    return 4 * (band_carve_floats(T, RB, W, h, w) + 8 + 4 * (1 << T))


def residual_lds_bytes(T, RB, W, h, w):
    return 4 * (band_carve_floats(T, RB, W, h, w) + 8 + 4)


def band_rows(c):
    """[(r0, r1)] of every band of a row; defect "r0_last": the last band starts one row early"""
    NB, RB = unroll_bands(c["R"], c["H"])
    return [(k * RB, min(k * RB + RB, c["H"])) for k in range(NB)]


# ---------------------------------------------------------------------------------------------------------------
# Pn: air_prune_score (and the rows air_propose_residual takes from it)
# ---------------------------------------------------------------------------------------------------------------
SC_MULT, SC_STD = 0.75, 0.3
RES_MULT, RES_HI = 0.5, 1.0


def _sc(H, W, h, w, T, R, reaches, **kw):
    return dict(H=H, W=W, h=h, w=w, T=T, R=R, reaches=reaches, off=kw.pop("off", {}), **kw)


SC_ROWS = {f"Sc_T{t}": _sc(6, 10, 3, 3, t, 2, f"prune_score_kernel<{t}>" + (" (first run)" if t in (2, 4) else "")) for t in range(1, 7)}
SC_ROWS.update({
    "Sc_21x19_planted": _sc(21, 19, 6, 10, 3, 2, "the planted transforms of group X; odd w: scalar staging", planted=True),
    "Sc_8x16": _sc(8, 16, 4, 4, 2, 3, "vec4 staging; eight one-row bands"),
    "Sc_8x16_glimpse_4B": _sc(8, 16, 4, 4, 2, 3, "glimpse 4 bytes off: scalar staging, the vector staging's bits", off={"glimpse": 1},
                              data="Sc_8x16"),
    "Sc_5x6": _sc(5, 6, 3, 3, 3, 1, "NB = H = 5, RB = 1"),
    "Sc_12x9_kinds": _sc(12, 9, 3, 3, 3, 5, "every presence kind at T = 3, where (1, 0, 1) has ones behind the chain"),
    "Sc_50x7": _sc(50, 7, 3, 3, 2, 1, "eight bands, the last a short one"),
    "Sc_33x32_one_band": _sc(33, 32, 4, 4, 2, 129, "one band of 1056 pixels: the second chunk holds 32, the prefetch clamps (first run)"),
    "Sc_65x32_one_band": _sc(65, 32, 4, 4, 1, 129, "one band of 2080 pixels: a third chunk (first run)"),
    "Sc_51x51_glimpse": _sc(6, 10, 51, 51, 6, 2, "a carve above 64 KiB: cv_allow_lds (first run)"),
})
RES_ROWS = ("Sc_33x32_one_band", "Sc_65x32_one_band", "Sc_51x51_glimpse", "Sc_21x19_planted", "Sc_8x16", "Sc_50x7", "Sc_12x9_kinds")


@functools.lru_cache(maxsize=None)
def sc_data(name):
    """glimpse [T, R, h, w], where [T, R, 4], presence [T, R] (image b of kind b % 5), obs [R, H, W]; finite everywhere"""
    c = SC_ROWS[name]
    if c.get("data"):
        return sc_data(c["data"])
    T, R, H, W, h, w = (c[k] for k in ("T", "R", "H", "W", "h", "w"))
    nref = min(R, N_REF)                                                   # the images past N_REF repeat the first ones and must repeat their bits
    rng = np.random.default_rng(_seed(name))
    glm = rng.uniform(0.05, 1.0, (T, nref, h, w)).astype(F32)
    where = WC.draw_where(T * nref, "write", H, W, h, w, rng).reshape(T, nref, 4)
    if c.get("planted"):
        rows = list(WC.planted_rows("write", H, W, h, w).values())
        for i, row in enumerate(rows[:T * nref - 1]):
            where.reshape(-1, 4)[i + 1] = row
    pres, n = np.empty((T, nref), F32), np.empty(nref, np.int64)
    for b in range(nref):
        pres[:, b], n[b] = presence_row(PRESENCE_KINDS[b % 5], T)
    obs = rng.uniform(0.0, 1.0, (nref, H, W)).astype(F32)
    rep = np.arange(R) % nref
    return dict(glimpse=glm[:, rep], where=np.ascontiguousarray(where[:, rep]), presence=pres[:, rep], obs=obs[rep], nref=nref, n=n[rep])


@functools.lru_cache(maxsize=None)
def sc_layers64(name):
    """float64 layers through warp_cases.warp64 -> (layers [T, nref, H, W], S_layers: the taps' magnitudes + the coordinate term)"""
    c = SC_ROWS[name]
    if c.get("data"):
        return sc_layers64(c["data"])
    d = sc_data(name)
    T, H, W, h, w, nref = c["T"], c["H"], c["W"], c["h"], c["w"], d["nref"]
    K = T * nref
    wh = d["where"][:, :nref].reshape(K, 4)
    ax, bx = WC.axis_ab(wh, "write", 0)
    ay, by = WC.axis_ab(wh, "write", 1)
    fw = WC.warp64(d["glimpse"][:, :nref].reshape(K, h, w).astype(F64), ax, bx, ay, by, W, H, np.zeros((K, H, W)))
    return fw["out"].reshape(T, nref, H, W), fw["S_out_coord"].reshape(T, nref, H, W)


def score_terms64(layers, S_layers, obs, m, mult, std, defect=None):
    """per pixel, mask m: the term 0.5 z^2 + cst and the three per-pixel parts of S (module docstring)"""
    T = layers.shape[0]
    canvas, S_c = np.zeros_like(layers[0]), np.zeros_like(layers[0])
    for t in range(T):
        if (m >> t) & 1:
            canvas, S_c = canvas + layers[t], S_c + S_layers[t]
    cst = 0.0 if defect == "no_cst" else HALF_LOG_2PI + np.log(std)
    z = (obs - mult * canvas) / std
    term = 0.5 * z * z + cst
    S1 = np.abs(z) * mult / std * WC.CONST["X"] * S_c
    S2 = z * z + np.abs(z) * (np.abs(obs) + mult * S_c) / std + np.abs(term)
    return term, S1 + S2, abs(cst)


def score_ref64(name, all_candidates, defect=None):
    """-> ref [NB, nref, 2^T] (NaN for the masks at or above 2^cb), S alike.  Defects: "drop_past_1024", "r0_last", "no_cst",
    "n_for_T" (n used where all_candidates asks for T)"""
    c, d = SC_ROWS[name], sc_data(name)
    T, H, W, nref = c["T"], c["H"], c["W"], d["nref"]
    layers, S_layers = sc_layers64(name)
    obs = d["obs"][:nref].astype(F64)
    mult, std = float(F32(SC_MULT)), float(F32(SC_STD))
    bands = band_rows(c)
    if defect == "r0_last" and len(bands) > 1:
        bands[-1] = (bands[-1][0] - 1, bands[-1][1])
    cb = np.where(all_candidates and defect != "n_for_T", T, d["n"][:nref])
    ref = np.full((len(bands), nref, 1 << T), NAN)
    S = np.full_like(ref, NAN)
    for m in range(1 << T):
        term, S_pix, acst = score_terms64(layers, S_layers, obs, m, mult, std, defect)
        live = m < (1 << cb)
        for k, (r0, r1) in enumerate(bands):
            npx = (r1 - r0) * W
            t_, s_ = term[:, r0:r1].reshape(nref, -1), S_pix[:, r0:r1].reshape(nref, -1)
            if defect == "drop_past_1024":
                t_ = t_[:, :1024]
            D = -(-npx // 256) + 6 + 3
            ref[k, live, m] = t_.sum(1)[live]
            S[k, live, m] = (s_.sum(1) + npx * acst + D * np.abs(t_).sum(1))[live]
    return ref, S


def thread_sum32(terms):
    """[.., npx] float32 -> the band's sum in the kernel's order: thread tid adds p = tid, tid + 256, .. in order, a butterfly inside
    each wave, the four wave totals added in wave order"""
    terms = np.asarray(terms, F32)
    npx = terms.shape[-1]
    P = -(-npx // 256)
    pad = np.zeros(terms.shape[:-1] + (P * 256,), F32)
    pad[..., :npx] = terms
    s = np.zeros(terms.shape[:-1] + (256,), F32)
    for p in range(P):
        live = np.arange(p * 256, p * 256 + 256) < npx
        s = np.where(live, (s + pad[..., p * 256:p * 256 + 256]).astype(F32), s)
    tot = np.zeros(terms.shape[:-1], F32)
    for wv in range(4):
        tot = (tot + butterfly(s[..., 64 * wv:64 * wv + 64])).astype(F32)
    return tot


def score_restate32(name, all_candidates):
    """prune_score_kernel in numpy float32 on the float32 layers of oracle/st_loops.c -> [NB, nref, 2^T]"""
    from oracle import st_loops as C
    c, d = SC_ROWS[name], sc_data(name)
    T, H, W, nref = c["T"], c["H"], c["W"], d["nref"]
    layers = np.stack([C.st_write_fwd(d["glimpse"][t, :nref], d["where"][t, :nref], (H, W)) for t in range(T)]).astype(F32)
    mult, std = F32(SC_MULT), F32(SC_STD)
    cst = F32(F32(0.5) * np.log(F32(6.283185307179586)) + np.log(std))
    cb = np.where(all_candidates, T, d["n"][:nref])
    bands = band_rows(c)
    out = np.full((len(bands), nref, 1 << T), NAN, F32)
    for m in range(1 << T):
        acc = np.zeros((nref, H, W), F32)
        for t in range(T):
            if (m >> t) & 1:
                acc = (acc + layers[t]).astype(F32)
        z = ((d["obs"][:nref] - mult * acc) / std).astype(F32)
        term = (F32(0.5) * z * z + cst).astype(F32)
        live = m < (1 << cb)
        for k, (r0, r1) in enumerate(bands):
            out[k, live, m] = thread_sum32(term[:, r0:r1].reshape(nref, -1))[live]
    return out


SC_REFUSALS = ([(k, {k: None}, -1) for k in ("glimpse", "where", "presence", "obs", "rec_sub")]
               + [("T=0", {"T": 0}, -2), ("T=7", {"T": 7}, -2), ("n_bands+1", {"bands": +1}, -2), ("n_bands-1", {"bands": -1}, -2),
                  ("where+4", {"bytes": ("where", 4)}, -3), ("glimpse+2", {"bytes": ("glimpse", 2)}, -3),
                  ("a carve above 160 KiB", {"h": 150, "w": 150}, -5)])


# ---------------------------------------------------------------------------------------------------------------
# Pr: air_propose_residual
# ---------------------------------------------------------------------------------------------------------------
def residual_rule(obs, recon, hi):
    """r = d > 0 ? min(d, hi) : 0 with d = obs - recon in float32 (recon = mult * canvas, air_parse_render's reconstruction): a NaN d
    gives 0; hi = +inf clamps nothing; a NaN hi clamps nothing either (fminf drops a NaN operand)"""
    with np.errstate(invalid="ignore"):
        d = (np.asarray(obs, F32) - np.asarray(recon, F32)).astype(F32)
        capped = d if np.isnan(hi) else np.minimum(d, F32(hi))
        return np.where(d > 0, capped, F32(0)).astype(F32)


def residual_ref64(name, counts=None, defect=None):
    """-> res64 [nref, H, W], its bound, the distance of d from the nearer clamp point minus the bound (<= 0: decided by the rule on
    the device's own canvas instead), parts64 [NB, nref] and its bound.  Defects: "ones_counted" (ones instead of leading ones),
    "no_clamp" """
    c, d = SC_ROWS[name], sc_data(name)
    T, W, nref = c["T"], c["W"], d["nref"]
    layers, S_layers = sc_layers64(name)
    mult, hi = float(F32(RES_MULT)), float(F32(RES_HI))
    n = d["n"][:nref] if counts is None else np.clip(np.asarray(counts)[:nref], 0, T)
    with np.errstate(invalid="ignore"):
        live = (d["presence"][:, :nref] > 0.5) if defect == "ones_counted" else (np.arange(T)[:, None] < n[None, :])
    live = live[:, :, None, None]
    canvas, S_c = np.where(live, layers, 0.0).sum(0), np.where(live, S_layers, 0.0).sum(0)
    obs = d["obs"][:nref].astype(F64)
    dd = obs - mult * canvas
    res = np.where(dd > 0, dd if defect == "no_clamp" else np.minimum(dd, hi), 0.0)
    bnd = RES_CONST * U * (np.abs(obs) + mult * S_c)
    clear = np.minimum(np.abs(dd), np.abs(dd - hi)) - bnd
    parts, pb = [], []
    for r0, r1 in band_rows(c):
        npx = (r1 - r0) * W
        r_, b_ = res[:, r0:r1].reshape(nref, -1), bnd[:, r0:r1].reshape(nref, -1)
        D = -(-npx // 256) + 6 + 3
        parts.append((r_ * r_).sum(1))
        pb.append((2.0 * r_ * b_ + b_ * b_).sum(1) + (D + 1) * U * (r_ * r_).sum(1))
    return dict(res=res, bound=bnd, clear=clear, parts=np.stack(parts), parts_bound=np.stack(pb))


RES_REFUSALS = ([(k, {k: None}, -1) for k in ("glimpse", "where", "obs", "res")] + [("presence and counts", {"presence": None}, -1)]
                + [("T=0", {"T": 0}, -2), ("T=7", {"T": 7}, -2), ("n_bands+1", {"bands": +1}, -2), ("where+4", {"bytes": ("where", 4)}, -3),
                   ("res+2", {"bytes": ("res", 2)}, -3), ("a carve above 160 KiB", {"h": 150, "w": 150}, -5)])


# ---------------------------------------------------------------------------------------------------------------
# Pn: air_prune_select
# ---------------------------------------------------------------------------------------------------------------
def _sel(T, R, A, G, bands, prior, reaches, off=None, data=None, allc=(0, 1), norm=1):
    off = dict(off or {})
    return dict(T=T, R=R, A=A, G=G, bands=bands, prior=prior, reaches=reaches, off=off, data=data, allc=allc, norm=norm,
                V=vec_rule(A, off.get("what", 0)))


SEL_ROWS = {
    "Sel_1x1x1x1": _sel(1, 1, 1, 1, 1, "fixed", "the smallest launch"),
    "Sel_3x5x12x16": _sel(3, 5, 12, 16, 3, "centred", "V = 4; R = 5 cuts the second workgroup after one wave"),
    "Sel_3x5x6x9": _sel(3, 5, 6, 9, 8, "fixed", "V = 2 by A", norm=0),
    "Sel_3x5x7x9": _sel(3, 5, 7, 9, 1, "centred", "V = 1 by A"),
    "Sel_6x4x8x4": _sel(6, 4, 8, 4, 1, "fixed", "64 masks: every lane live"),
    "Sel_6x257x50x16": _sel(6, 257, 50, 16, 3, "centred", "65 workgroups, the last with one wave", norm=0),
    "Sel_3x5x12x16_what_4B": _sel(3, 5, 12, 16, 3, "centred", "V = 1 by the alignment of what (first run)", {"what": 1}, "Sel_3x5x12x16"),
    "Sel_3x5x12x16_what_8B": _sel(3, 5, 12, 16, 3, "centred", "V = 2 by the alignment of what (first run)", {"what": 2}, "Sel_3x5x12x16"),
    "Sel_3x5x12x16_what_out_4B": _sel(3, 5, 12, 16, 3, "centred", "the word copy of what", {"what_out": 1}, "Sel_3x5x12x16"),
    "Sel_3x5x12x16_glimpse_out_4B": _sel(3, 5, 12, 16, 3, "centred", "the word copy of glimpse", {"glimpse_out": 1}, "Sel_3x5x12x16"),
}


@functools.lru_cache(maxsize=None)
def sel_data(name):
    """float32 rows, rec_sub [bands, R, 2^T] planted (an input here), a count table that does not sum to 1.  One what element per image
    holds the payload NaN behind n where there is such a row (all_candidates = 0 never reads it; the copy keeps it), one -0.0"""
    c = SEL_ROWS[name]
    if c["data"]:
        return sel_data(c["data"])
    T, R, A, G = c["T"], c["R"], c["A"], c["G"]
    rng = np.random.default_rng(_seed(name))
    nrm = lambda *s: rng.standard_normal(s).astype(F32)
    pres, n = np.empty((T, R), F32), np.empty(R, np.int64)
    for r in range(R):
        pres[:, r], n[r] = presence_row(PRESENCE_KINDS[r % 5], T)
    where = np.stack([rng.uniform(0.3, 1.2, (T, R)), rng.uniform(-0.8, 0.8, (T, R))] * 2, -1).astype(F32)
    d = dict(what=F32(0.3) + F32(1.2) * nrm(T, R, A), where=where, where_loc=(where + F32(0.1) * nrm(T, R, 4)).astype(F32),
             glimpse=rng.uniform(0, 1, (T, R, G)).astype(F32), score=rng.uniform(0, 1, (T, R)).astype(F32), presence=pres, n=n,
             rec_sub=rng.uniform(5.0, 60.0, (c["bands"], R, 1 << T)).astype(F32), prior=rng.uniform(0.05, 1.0, T + 1))
    d["glimpse"][0, :, 0] = F32(-0.0)
    d["score"][T - 1, :] = np.array([PAYLOAD_BITS], np.uint32).view(F32)[0]
    return d


def sel_ref64(d, c, pr, all_candidates, norm=None, defect=None):
    """float64 on the float32 inputs -> J [R, 2^T] (NaN for the masks at or above 2^cb), S alike, n.  Defect "prior_unnormalised" """
    T, R, A = d["what"].shape
    V = c["V"]
    n = leading_ones(d["presence"])
    cb = np.full(R, T) if all_candidates else n
    mu, sd = where_prior(d["where_loc"], pr, d["where"].shape)
    lw, Sw = _ln64(d["what"], pr[0], pr[1])
    lh, Sh = _ln64(d["where"], mu, sd)
    lp, S_lp = lw.sum(-1) + lh.sum(-1), depth(A // V) * (Sw.sum(-1) + Sh.sum(-1))
    rec = f32_band_sum(d["rec_sub"]).astype(F64)
    norm = c["norm"] if norm is None else norm
    total = 1.0
    if norm and defect != "prior_unnormalised":
        total = 0.0
        for v in d["prior"]:
            total += float(v)
    J, S = np.full((R, 1 << T), NAN), np.full((R, 1 << T), NAN)
    with np.errstate(all="ignore"):
        log_pi = np.log(np.asarray(d["prior"], F64) / total)
        for m in range(1 << T):
            lat, S_lat = np.zeros(R), np.zeros(R)
            for t in range(T):
                if (m >> t) & 1:
                    lat, S_lat = lat + lp[t], S_lat + S_lp[t]
            live = m < (1 << cb)
            k = bin(m).count("1")
            J[live, m] = ((-rec[:, m] + lat) + log_pi[k])[live]
            S[live, m] = (S_lat + np.abs(rec[:, m]) + (np.abs(log_pi[k]) if np.isfinite(log_pi[k]) else 0.0))[live]
    return J, S, n


def sel_restate32(d, c, pr, all_candidates, V):
    """prune_select_kernel<V> in numpy: the float32 latent term of every step in its lane layout, the closing adds in float64"""
    T, R, A = d["what"].shape
    pr32 = [F32(v) for v in pr]
    AV = A // V
    n = leading_ones(d["presence"])
    centred = np.isnan(pr32[4])
    J = np.full((R, 1 << T), NAN)
    with np.errstate(all="ignore"):
        l_w, l_s, l_h = np.log(pr32[1]), np.log(pr32[3]), np.log(pr32[5])
        total = 1.0
        if c["norm"]:
            total = 0.0
            for v in d["prior"]:
                total += float(v)
        rec = f32_band_sum(d["rec_sub"])
        for r in range(R):
            cb = T if all_candidates else int(n[r])
            lp = np.zeros(T)
            for t in range(cb):
                wt = _ln32(d["what"][t, r, :AV * V], pr32[0], pr32[1], l_w)
                loc = np.array([pr32[2], d["where_loc"][t, r, 1] if centred else pr32[4], pr32[2],
                                d["where_loc"][t, r, 3] if centred else pr32[4]], F32)
                ht = _ln32(d["where"][t, r], loc, np.array([pr32[3], pr32[5], pr32[3], pr32[5]], F32), np.array([l_s, l_h, l_s, l_h], F32))
                lp[t] = float(RC._row_sum32(wt, ht[None], 1, AV, V))
            for m in range(1 << cb):
                lat = 0.0
                for t in range(T):
                    if (m >> t) & 1:
                        lat += lp[t]
                J[r, m] = (-float(rec[r, m]) + lat) + np.log(float(d["prior"][bin(m).count("1")]) / total)
    return J


def visit(J, n, T, all_candidates, defect=None):
    """the visiting rule on one image's joints: the start mask first, then from the full mask down, strict; a NaN never wins.
    Defects: "tie_to_smaller" (>= on the way down), "start_not_first" (the plain downward visit)"""
    cb = T if all_candidates else n
    m0 = (1 << n) - 1
    order = [m0] + [m for m in range((1 << cb) - 1, -1, -1) if m != m0]
    if defect == "start_not_first":
        order = list(range((1 << cb) - 1, -1, -1))
    bm, best, have = m0, NAN, False
    for m in order:
        v = float(J[m])
        if np.isnan(v):
            continue
        if not have or v > best or (defect == "tie_to_smaller" and v == best):
            bm, best, have = m, v, True
    return bm


SEL_PLANTED = ("twins_tie", "start_ties", "all_nan", "start_nan", "one_pinf", "plain", "twins_tie_n3", "plain2")
SEL_PLANTED_ROW = dict(T=3, R=len(SEL_PLANTED), A=8, G=4, bands=2, prior="fixed", off={}, V=4, norm=1, data=None)


@functools.lru_cache(maxsize=None)
def sel_planted_data():
    """all_candidates = 1, T = 3, the count table (0.3, 0.5, 0.0, 0.4): every mask of two steps is -inf.  Image by SEL_PLANTED:
    twins_tie     steps 0 and 1 hold identical rows and masks 1 and 2 equal, lowest shares, the start mask is 0 (presence 0, ..): J[1] and
                  J[2] are equal to the bit and above every other; from the full mask down mask 2 comes first and `>` keeps it;
    start_ties    the same twins with presence (1, 0, 1): the start mask is 1 and ties with mask 2: the start mask stays;
    all_nan       every share NaN: best_mask = m0 = 7, the objective NaN;
    start_nan     the share of the start mask (7) alone NaN: the visit skips it;
    one_pinf      the share of mask 4 is -inf: J[4] = +inf wins;
    twins_tie_n3  the twins with every step present (m0 = 7): mask 2 again"""
    c = SEL_PLANTED_ROW
    T, R, A, G = c["T"], c["R"], c["A"], c["G"]
    rng = np.random.default_rng(_seed("sel_planted"))
    nrm = lambda *s: rng.standard_normal(s).astype(F32)
    where = np.stack([rng.uniform(0.3, 1.2, (T, R)), rng.uniform(-0.8, 0.8, (T, R))] * 2, -1).astype(F32)
    d = dict(what=F32(0.3) + nrm(T, R, A), where=where, where_loc=where.copy(), glimpse=rng.uniform(0, 1, (T, R, G)).astype(F32),
             score=rng.uniform(0, 1, (T, R)).astype(F32), presence=np.ones((T, R), F32),
             rec_sub=rng.uniform(40.0, 60.0, (c["bands"], R, 1 << T)).astype(F32), prior=np.array([0.3, 0.5, 0.0, 0.4]))
    for tag in ("twins_tie", "start_ties", "twins_tie_n3"):
        r = SEL_PLANTED.index(tag)
        d["what"][1, r], d["where"][1, r], d["where_loc"][1, r] = d["what"][0, r], d["where"][0, r], d["where_loc"][0, r]
        d["rec_sub"][:, r, 1] = d["rec_sub"][:, r, 2] = F32(1.5)
    d["presence"][:, SEL_PLANTED.index("twins_tie")] = 0.0
    d["presence"][1, SEL_PLANTED.index("start_ties")] = 0.0
    d["rec_sub"][:, SEL_PLANTED.index("all_nan")] = NAN
    d["rec_sub"][1, SEL_PLANTED.index("start_nan"), 7] = NAN
    d["rec_sub"][0, SEL_PLANTED.index("one_pinf"), 4] = -np.inf
    d["n"] = leading_ones(d["presence"])
    return d


SEL_PLANTED_MASKS = {"twins_tie": 2, "start_ties": 1, "all_nan": 7, "one_pinf": 4, "twins_tie_n3": 2}

SEL_IN = ("what", "where", "glimpse", "score", "presence", "where_loc", "prior", "rec_sub")
SEL_OUT = ("J_sub", "best_mask", "num_objects_out", "kept_step", "objective", "objective_start", "evidence", "what_out", "where_out",
           "glimpse_out", "score_out")
SEL_REFUSALS = ([(k, {k: None}, -1) for k in SEL_IN if k != "where_loc"] + [(k, {k: None}, -1) for k in SEL_OUT]
                + [("where_loc under a NaN shift loc", {"where_loc": None}, -1)]
                + [("T=0", {"T": 0}, -2), ("T=7", {"T": 7}, -2), ("n_bands=0", {"bands": 0}, -2), ("n_bands=9", {"bands": 9}, -2)]
                + [(k + "+4", {"bytes": (k, 4)}, -3) for k in ("where", "where_out", "where_loc", "prior", "J_sub", "objective",
                                                               "objective_start", "evidence")])


# ---------------------------------------------------------------------------------------------------------------
# Pr: air_propose_pool, air_propose_source
# ---------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1), (3, 3, 5), (5, 1, 257), (2, 1, 6)]               # (T, P, R)
POOL_WIDTHS = [(8, 16), (7, 9)]                                            # (A, G)


@functools.lru_cache(maxsize=None)
def pool_data(T, P, R, A, G):
    rng = np.random.default_rng(_seed(f"pool{T}{P}{R}{A}{G}"))
    f = lambda *s: rng.standard_normal(s).astype(F32)
    d = dict(what=f(T, R, A), where=f(T, R, 4), glimpse=f(T, R, G), score=f(T, R), prop_what=f(T, R, A), prop_where=f(T, R, 4),
             prop_glimpse=f(T, R, G), prop_score=f(T, R), prior=rng.uniform(0.05, 1.0, T + 1),
             counts=rng.integers(-3, T + 4, R).astype(np.int32), source_in=rng.integers(0, 50, (T, R)).astype(np.int32))
    pres = np.empty((T, R), F32)
    for r in range(R):
        pres[:, r] = presence_row(PRESENCE_KINDS[r % 5], T)[0]
    d["presence"] = pres
    d["what"][0, 0, 0] = np.array([PAYLOAD_BITS], np.uint32).view(F32)[0]
    d["prop_glimpse"][0, 0, G - 1] = F32(-0.0)
    return d


POOL_REFUSALS = ([(k, {k: None}, -1) for k in ("what", "where", "glimpse", "score", "prop_what", "prop_where", "prop_glimpse", "prop_score",
                                                "prior", "pool_what", "pool_where", "pool_glimpse", "pool_score", "pool_presence",
                                                "pool_source", "pool_prior")]
                 + [("presence and counts", {"presence": None}, -1), ("P=0", {"P": 0}, -2), ("P>T", {"T": 2, "P": 3}, -2),
                    ("T+P=7", {"T": 4, "P": 3}, -2), ("round=-1", {"round": -1}, -2), ("prior+4", {"bytes": ("prior", 4)}, -3),
                    ("pool_prior+4", {"bytes": ("pool_prior", 4)}, -3)])


# ---------------------------------------------------------------------------------------------------------------
# coverage: the fourteen kernels of the three files, and the rows that name them
# ---------------------------------------------------------------------------------------------------------------
INSTANTIATIONS = (tuple(f"refine_step_kernel<{v}>" for v in (4, 2, 1)) + tuple(f"prune_score_kernel<{t}>" for t in range(1, 7))
                  + tuple(f"prune_select_kernel<{v}>" for v in (4, 2, 1))
                  + ("propose_residual_kernel", "propose_pool_kernel", "propose_source_kernel"))


def named_instantiations():
    names = {f"refine_step_kernel<{c['V']}>" for c in RF_ROWS.values()}
    names |= {f"prune_score_kernel<{c['T']}>" for c in SC_ROWS.values()}
    names |= {f"prune_select_kernel<{c['V']}>" for c in SEL_ROWS.values()}
    if all(r in SC_ROWS for r in RES_ROWS):
        names.add("propose_residual_kernel")
    if POOL_SHAPES:
        names |= {"propose_pool_kernel", "propose_source_kernel"}
    return names
