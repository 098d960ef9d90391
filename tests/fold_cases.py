"""Case builders and float64 references for the kernel-level tests of the launches folded into the train step
(tests/test_fold_kernels.py): air_gemm_grouped_opt, air_gemm_grouped_gauss_bwd, the HBM feeder (air_batch_gather,
air_gemm_grouped_gather, air_step_prologue_gather_cvt), the step prologue on its own and riding on the first LSTM step
(air_step_prologue[_cvt], air_lstm_step_fwd_prologue, air_lstm_first_step_fwd) and the small riders (air_canvas_unroll_bwd_dpresence /
_nvil, air_sum_leading, air_l2_grad_add, air_counter_add).  Importable without a GPU; tests/test_fold_cases_host.py builds every case
on the CPU, holds it against the host mirror of the dispatch rules (attend_infer_repeat_amd/gemm_groups.py) and checks the references
against independent ones.  No test lives here.

Every builder is cached and returns float32 inputs with float64 expectations as CPU tensors.  Conditions a comparison relies on are
asserted where the input is made:
  * ms - mg^2 >= 0.1 in every optimiser state (the update keeps decay * (ms - mg^2) of it: the square root never sees a cancellation);
  * no ELU output within 1e-3 of 0 (the kink of elu'), no floored scale but the one row meant to be floored;
  * fold regions and rider ranges start at multiples of 4 and are pairwise disjoint; rider ranges end at multiples of 4;
  * n_model strictly inside the fold region of the case that straddles it;
  * every reference is finite."""
import functools

import numpy as np
import torch

from oracle import air_oracle as O

from attend_cases import SENTINEL, WORST, _elu_output, _rounded, assert_bits, assert_close, elu_prime, g, print_worst, rand_where  # noqa: F401

F32, BF16 = 0, 1
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------
# Philox4x32-10 on the host (csrc/prologue_device.h philox4x32: counter = {ctr lo, ctr hi, stream lo, stream hi}, key = {seed lo, seed hi})
# ---------------------------------------------------------------------------------------------------------------
def philox4x32(ctr, stream, seed):
    """one block in Python integers -> [r0, r1, r2, r3]"""
    c = [ctr & M32, (ctr >> 32) & M32, stream & M32, (stream >> 32) & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def philox4x32_np(ctr, stream, seed):
    """the same for an array of 64-bit counters (uint64, wrapping) -> uint32 [n, 4]"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    m = np.uint64(M32)
    c = [ctr & m, ctr >> np.uint64(32), np.full_like(ctr, stream & M32), np.full_like(ctr, (stream >> 32) & M32)]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & m, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, 1).astype(np.uint32)


# Random123's published known answers for philox4x32_10 (kat_vectors): (counter words, key words, output words)
PHILOX_KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_normals(seed, offset, n):
    """what air_rng_fill(normal, n, NULL, 0, {seed, offset}) writes (drawn on the device: needs a GPU)"""
    from attend_infer_repeat_amd import hip as H
    z = torch.zeros(n, device="cuda")
    H.rng_fill(torch.tensor([seed, offset], dtype=torch.int64, device="cuda"), normal=z, advance=False)
    torch.cuda.synchronize()
    return z


def noise_ref(seed, offset, n_normal, n_uniform):
    """what the step prologue draws at state {seed, offset}: quads of normals first (counter offset + q, stream 0), then quads of
    uniforms.  uniform[4 q + k] = u01(r[k]) = (r[k] >> 8) * 2^-24, exact in float32.  normal[4 q + 2 k], [4 q + 2 k + 1] =
    rad * cos(th), rad * sin(th) with rad = sqrt(-2 log(u1)), th = 2 pi u2 on the float32 values u1 = u01_open(r[2k]) =
    ((r[2k] >> 8) + 0.5f) * 2^-24 and u2 = u01(r[2k+1]), everything from there on in float64 -- the angle too, which the kernel forms
    as a float32 product (NORMAL_TOL accounts for that rounding).
    -> normal64[n_normal], uniform32[n_uniform]"""
    qn, qu = (n_normal + 3) // 4, (n_uniform + 3) // 4
    ctr = (np.arange(qn + qu, dtype=np.uint64) + np.uint64(offset & 0xFFFFFFFFFFFFFFFF))
    r = philox4x32_np(ctr, 0, seed)
    scale = np.float32(1.0 / 16777216.0)
    rn = r[:qn]
    u1 = ((rn[:, 0::2] >> 8).astype(np.float32) + np.float32(0.5)) * scale                  # [qn, 2], float32 like the kernel
    u2 = (rn[:, 1::2] >> 8).astype(np.float32) * scale                                      # exact
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    rad, th = np.sqrt(-2.0 * np.log(u1.astype(np.float64))), 2.0 * np.pi * u2.astype(np.float64)
    z = np.stack([rad * np.cos(th), rad * np.sin(th)], -1).reshape(qn, 4)
    u = ((r[qn:] >> 8).astype(np.float32) * scale).reshape(-1)
    return torch.as_tensor(z.reshape(-1)[:n_normal].copy()), torch.as_tensor(u[:n_uniform].copy())


def feeder_indices(seed, step, B, n_items, shuffle):
    """idx_b of air_batch_gather in Python integers: (((r0 << 32) | r1) * n_items) >> 64 with Philox(counter step * B + b, stream 1,
    seed), or (step * B + b) mod n_items for the sequential walk; the counter wraps at 2^64"""
    out = []
    for b in range(B):
        ctr = (step * B + b) & 0xFFFFFFFFFFFFFFFF
        if shuffle:
            r = philox4x32(ctr, 1, seed)
            out.append((((r[0] << 32) | r[1]) * n_items) >> 64)
        else:
            out.append(ctr % n_items)
    return out


def prior_ref(anneal, init, final, steps, hold, div, gstep, T):
    """the annealed geometric prior table through the oracle's own schedule (float64)"""
    s = init if anneal is None else O.anneal_weight(init, final, anneal, gstep, steps, hold, div)
    return O.geometric_prior(s, T)


# anneal_type, init, final, anneal_steps, hold_for, steps_div and three device step counts: below hold_for, midway, past the floor
PRIOR_SCHEDULES = [
    (None, 0.3, 0.0, 1.0, 0.0, 1.0, (0, 500, 100000)),
    ("exp", 0.9, 1e-3, 1000.0, 100.0, 10.0, (50, 600, 100000)),
    ("linear", 0.9, 1e-3, 1000.0, 100.0, 1.0, (50, 600, 100000)),
]


# ---------------------------------------------------------------------------------------------------------------
# shared references
# ---------------------------------------------------------------------------------------------------------------
def f32v(x):
    """the float32 value of a Python number, as a Python float: what a kernel is handed for a float argument"""
    return float(np.float32(x))


def product64(A, B, ta, tb, precision):
    """op(A) . op(B) in float64 on the float32 operands (rounded to bf16 first for precision 1)"""
    r = _rounded(precision)
    a, b = r(A).double(), r(B).double()
    return (a.t() if ta else a) @ (b.t() if tb else b)


def product_tol(K):
    """the bound of test_gemm_all_layouts: 1e-5 relative + 8e-6 sqrt(K) absolute"""
    return 1e-5, 8e-6 * K ** 0.5


def rmsprop64(p, grad, ms, mg, mom, lr, decay, momentum, eps, grad_scale):
    """rmsprop_elem (csrc/optimizer_device.h) in float64 on float32 inputs; lr may be a tensor (two learning rates); the float
    hyperparameters enter with their float32 values.  -> p, ms, mg, mom"""
    d, m, e, s = f32v(decay), f32v(momentum), f32v(eps), f32v(grad_scale)
    gi = grad.double() * s
    msi = d * ms.double() + (1.0 - d) * gi * gi
    mgi = d * mg.double() + (1.0 - d) * gi
    mo = m * mom.double() + torch.as_tensor(lr, dtype=torch.float64) * gi / torch.sqrt(msi - mgi * mgi + e)
    return p.double() - mo, msi, mgi, mo


# The bound of test_rmsprop_centered, 1e-6 relative + 1e-7 absolute, for p, ms and mom.  For mg it was set where it cannot bind (from
# mg = 0 there is no cancellation); here mg' = d mg + (1 - d) g lands near 0 for some elements while its two terms, with gradients up
# to 35, stay O(1): the error is a float32 ulp of the terms, not of the result.  Measured on the UNFUSED pair (air_gemm_grouped +
# air_step_epilogue, to which the folded launch is bit-equal) against the same float64 reference over all nine runs: worst error /
# (1e-6 |ref| + 1e-7) = 1.056 for mg (32 x 32 tiles, bf16; 1.021 on the streaming body), 0.22 / 0.15 / 0.34 for p / ms / mom.  One
# run of one seed is a sample: mg is allowed twice what was measured, 2 x 1.056 = 2.112 of the borrowed bound.
RMS_TOL = {"p": (1e-6, 1e-7), "ms": (1e-6, 1e-7), "mg": (2.112e-6, 2.112e-7), "mom": (1e-6, 1e-7)}


def lstm64(h_prev, c_prev, w_h, gx, forget_bias, precision):
    """one LSTM step in float64 (Sonnet gate order i, j, f, o): gates = h_prev . w_h + gx; h_prev / c_prev may be one broadcast row"""
    r = _rounded(precision)
    g64 = r(h_prev).double() @ r(w_h).double() + gx.double()
    i, j, f, o = torch.chunk(g64, 4, -1)
    gi, gj, gf, go = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + forget_bias), torch.sigmoid(o)
    c = gf * c_prev.double() + gi * gj
    return torch.tanh(c) * go, c, torch.cat([gi, gj, gf, go], -1)


LSTM_TOL = (2e-5, 2e-5)


# ---------------------------------------------------------------------------------------------------------------
# G. air_gemm_grouped_opt
# ---------------------------------------------------------------------------------------------------------------
# problems: (M, N, K, colsum, folded) -- TN weight gradients dW[M, N] = X[K, M]^T . dY[K, N]; ranges: rider slices as lengths (0 = an
# empty one); straddle: n_model falls inside the first folded C; counters: the launch advances the step counter and the Philox offset
OPT_CASES = {
    "tile16": dict(problems=[(37, 50, 64, True, True), (100, 20, 64, False, False)], ranges=[40, 0], form=(1, 1, 4)),
    "wave16": dict(problems=[(20, 48, 520, True, True)], ranges=[], form=(1, 1, 16)),
    "tile32": dict(problems=[(800, 500, 24, True, True)], ranges=[64], form=(2, 2, 4)),
    "shortk": dict(problems=[(4099, 64, 16, True, True), (6163, 192, 48, True, True)], ranges=[24], form="shortk"),
    "straddle": dict(problems=[(37, 50, 64, True, True), (100, 20, 64, False, True)], ranges=[40, 0, 8, 132], form=(1, 1, 4),
                     straddle=True, grad_scale=0.5),
    "early": dict(problems=[(37, 50, 64, True, True), (100, 20, 64, False, False)], ranges=[], form=(1, 1, 4), counters=False),
}
OPT_RUNS = [("tile16", F32), ("tile16", BF16), ("wave16", F32), ("wave16", BF16), ("tile32", F32), ("tile32", BF16), ("shortk", F32),
            ("straddle", F32), ("early", F32)]
# declined with AIR_E_UNSUPPORTED, nothing written: a short-K problem mixed with a tile problem; an all-TN group of more than
# wide_min_tiles() = 1000 tiles with K >= 256
OPT_DECLINED = {
    "shortk_mixed": [(4099, 64, 16, False, True), (37, 50, 64, False, True)],
    "wide_regime": [(512, 512, 256, False, True)],
}
OPT_HYPER = dict(lr=1e-2, lr_mult_tail=0.25, decay=0.9, momentum=0.9, eps=1e-10)
RNG_INCREMENT = 12345


def _pad4(n):
    return (n + 3) // 4 * 4


def _opt_layout(problems, ranges):
    """offsets into the flat buffers: [gap | C_0 | gap | colsum_0 | ... | gap | range_0 | gap | ...]; every start a multiple of 4, a gap
    of at least 4 sentinels in front of and behind everything -> (regions of the folded problems, rider (lo, hi), n_total)"""
    off, c_off, cs_off, rng = 4, [], [], []
    for (M, N, K, colsum, folded) in problems:
        if folded:
            c_off.append(off); off = _pad4(off + M * N) + 4
            cs_off.append(off if colsum else None)
            if colsum:
                off = _pad4(off + N) + 4
        else:
            c_off.append(None); cs_off.append(None)
    for n in ranges:
        rng.append((off, off + n)); off = off + n + 4
    return c_off, cs_off, rng, off


@functools.lru_cache(maxsize=None)
def opt_case(name, precision=F32, declined=False):
    spec = dict(problems=OPT_DECLINED[name], ranges=[8], form=None) if declined else OPT_CASES[name]
    seed = sum(ord(ch) for ch in name) * 7 + precision
    gen = torch.Generator().manual_seed(seed)
    c = dict(name=name, precision=precision, form=spec["form"], grad_scale=spec.get("grad_scale", 1.0),
             counters=spec.get("counters", True), **OPT_HYPER)
    c_off, cs_off, ranges, n_total = _opt_layout(spec["problems"], spec["ranges"])
    c.update(c_off=c_off, cs_off=cs_off, ranges=ranges, n_total=n_total)
    c["problems"] = []
    for i, (M, N, K, colsum, folded) in enumerate(spec["problems"]):
        X = torch.randn(K, M, generator=gen); dY = torch.randn(K, N, generator=gen)
        c["problems"].append(dict(M=M, N=N, K=K, colsum=colsum, folded=folded, X=X, dY=dY,
                                  C64=product64(X, dY, True, False, precision), colsum64=dY.double().sum(0) if colsum else None))
    c["fold_mask"] = sum(1 << i for i, pr in enumerate(c["problems"]) if pr["folded"])
    # regions the launch updates: folded C / colsum, rider ranges
    fold_regions = []
    for i, pr in enumerate(c["problems"]):
        if pr["folded"]:
            fold_regions.append((c_off[i], c_off[i] + pr["M"] * pr["N"]))
            if pr["colsum"]:
                fold_regions.append((cs_off[i], cs_off[i] + pr["N"]))
    c["fold_regions"] = fold_regions
    if spec.get("straddle"):
        lo, hi = fold_regions[0]
        c["n_model"] = _pad4((lo + hi) // 2)
        assert lo < c["n_model"] < hi and c["n_model"] % 4 == 0
    else:
        c["n_model"] = _pad4(n_total)                       # (one learning rate)
    regions = fold_regions + [r for r in ranges]
    for a0, a1 in regions:
        assert a0 % 4 == 0 and 0 < a0 <= a1 <= n_total - 4
    for (a0, a1) in ranges:
        assert a1 % 4 == 0
    srt = sorted(r for r in regions if r[1] > r[0])
    assert all(srt[k][1] <= srt[k + 1][0] for k in range(len(srt) - 1)), "regions overlap"
    # the optimiser state: ms - mg^2 >= 0.1
    c["p"] = torch.randn(n_total, generator=gen)
    c["mg"] = torch.randn(n_total, generator=gen) * 0.5
    c["ms"] = (c["mg"].double() ** 2 + 0.1 + 0.1 + torch.rand(n_total, generator=gen).double()).float()
    c["mom"] = torch.randn(n_total, generator=gen) * 0.01
    assert bool((c["ms"].double() - c["mg"].double() ** 2 >= 0.1).all())
    # the gradient buffer: a sentinel everywhere, final gradients in the rider ranges; the folded regions are NaN-primed by the test
    c["g"] = torch.full((n_total,), SENTINEL)
    for a0, a1 in ranges:
        c["g"][a0:a1] = torch.randn(a1 - a0, generator=gen)
    touched = torch.zeros(n_total, dtype=torch.bool)
    for a0, a1 in regions:
        touched[a0:a1] = True
    c["touched"] = touched
    lr0 = np.float32(c["lr"])
    lr = torch.full((n_total,), float(lr0), dtype=torch.float64)
    lr[c["n_model"]:] = float(lr0 * np.float32(c["lr_mult_tail"]))
    c["lr_elem"] = lr
    for pr in c["problems"]:
        assert bool(torch.isfinite(pr["C64"]).all())
    return c


def opt_descs(c, base=1 << 20):
    """the case as AirGemmDesc-like records at made-up 16-byte aligned addresses (for the host mirror of the dispatch rules)"""
    from attend_infer_repeat_amd import _lib
    out = []
    for pr in c["problems"]:
        out.append(_lib.AirGemmDesc(1, 0, pr["M"], pr["N"], pr["K"], base, pr["M"], base, pr["N"], base, pr["N"], None, 0, None, 0, 0.0,
                                    base if pr["colsum"] else None, c["precision"], None, None, 0, None))
    return out


# ---------------------------------------------------------------------------------------------------------------
# H. air_gemm_grouped_gauss_bwd
# ---------------------------------------------------------------------------------------------------------------
GB_OFFSET, GB_PRIOR, GB_DKL_SCALE = 0.5, (0.1, 1.3), 0.7
# form: M, D, K of the dsample product, its index in the group, the other problems
GB_FORMS = {
    "tile4": dict(M=37, D=50, K=256, problem=1, others=True, form=(1, 1, 4)),
    "wave16": dict(M=20, D=48, K=520, problem=0, others=False, form=(1, 1, 16)),
}
# form, precision, dkl_row given, NVIL rider (n_parts, B) | None, KL-share rider (parts) | 0, guard_eps
GB_RUNS = [
    ("tile4", F32, True, (4, 130), 7, 0.0),
    ("tile4", F32, False, None, 0, 0.0),
    ("tile4", F32, True, (1, 1), 0, 1e-3),
    ("tile4", BF16, True, None, 3, 0.0),
    ("wave16", F32, True, (4, 1), 6, 0.0),
    ("wave16", F32, False, (1, 130), 0, 0.0),
    ("wave16", BF16, True, (1, 130), 1, 0.0),
]
GB_DECLINED = dict(M=37, D=50, K=256, extra=(1000, 256, 16))          # 3 * 4 + 63 * 16 = 1020 tiles > 1000


def gauss_head64(pre, eps, guard_eps=0.0):
    """pre[M, 2D], eps[M, D] in float64 -> sample, kl_row (loc_mode 0, one prior): the forward of test_gauss_sample_fwd_bwd"""
    D = eps.shape[1]
    loc = pre[:, :D]
    scale = O._guard_scale(O.softplus(pre[:, D:] + GB_OFFSET), guard_eps)
    pl, ps = (torch.tensor(v, dtype=torch.float64) for v in GB_PRIOR)
    return loc + scale * eps, O.normal_kl(loc, scale, pl, ps).sum(-1), loc, scale


def gauss_dpre64(pre, eps, dsample, dkl_row, guard_eps=0.0):
    """float64 autograd of sum(sample * dsample) + dkl_scale * sum(dkl_row * kl_row) at the float32 pre the kernel is handed"""
    p64 = pre.double().requires_grad_(True)
    sample, kl, _, _ = gauss_head64(p64, eps.double(), guard_eps)
    L = (sample * dsample.double()).sum()
    if dkl_row is not None:
        L = L + f32v(GB_DKL_SCALE) * (dkl_row.double() * kl).sum()
    gp, = torch.autograd.grad(L, [p64])
    return gp


def gauss_dpre_by_hand(pre, eps, dsample, dkl_row):
    """the same gradient written out (guard off): d loc = dsample + dkl (loc - p_loc) / p_scale^2,
    d raw = sigmoid(raw + offset) * (dsample * eps + dkl (scale / p_scale^2 - 1 / scale))"""
    D = eps.shape[1]
    p = pre.double()
    loc, raw = p[:, :D], p[:, D:] + GB_OFFSET
    scale = torch.nn.functional.softplus(raw)
    dk = f32v(GB_DKL_SCALE) * dkl_row.double()[:, None] if dkl_row is not None else torch.zeros(p.shape[0], 1, dtype=torch.float64)
    pl, ps = GB_PRIOR
    return torch.cat([dsample.double() + dk * (loc - pl) / ps ** 2,
                      torch.sigmoid(raw) * (dsample.double() * eps.double() + dk * (scale / ps ** 2 - 1.0 / scale))], 1)


@functools.lru_cache(maxsize=None)
def gb_case(i):
    form, precision, has_dkl, nvil, n_kl, guard = GB_RUNS[i]
    f = GB_FORMS[form]
    M, D, K = f["M"], f["D"], f["K"]
    gen = torch.Generator().manual_seed(6000 + i)
    c = dict(form=f["form"], precision=precision, M=M, D=D, K=K, problem=f["problem"], guard=guard, n_kl=n_kl, nvil=nvil,
             ld_pre=2 * D + 4, ld_dpre=2 * D + 8)
    c["gy"] = torch.randn(M, K, generator=gen) / K ** 0.5                     # dsample = gy . W^T
    c["W"] = torch.randn(D, K, generator=gen)
    c["dsample64"] = product64(c["gy"], c["W"], False, True, precision)
    c["pre"] = torch.randn(M, 2 * D, generator=gen)
    c["eps"] = torch.randn(M, D, generator=gen)
    c["dkl_row"] = torch.randn(M, generator=gen) if has_dkl else None
    if guard > 0:
        c["pre"][0, D] = -12.0 - GB_OFFSET                                      # one scale under the floor, no other near it
    s64 = O.softplus(c["pre"].double()[:, D:] + GB_OFFSET)
    assert int((s64 < max(guard, 1e-30) * 2).sum()) == (1 if guard > 0 else 0) and bool((s64 > 0).all())
    _, kl, loc, scale = gauss_head64(c["pre"].double(), c["eps"].double(), guard)
    c["loc"], c["scale"] = loc.float(), scale.float()                           # what the forward would have stored
    c["others"] = []
    if f["others"]:
        # a TN weight gradient in front, an NT product with the ELU' epilogue behind
        X = torch.randn(64, 33, generator=gen); dY = torch.randn(64, 20, generator=gen)
        c["others"].append(dict(kind="tn", A=X, B=dY, ta=True, tb=False, K=64, ref=product64(X, dY, True, False, precision)))
        A = torch.randn(21, 40, generator=gen); B = torch.randn(70, 40, generator=gen); y = _elu_output(gen, 21, 70)
        c["others"].append(dict(kind="nt_delu", A=A, B=B, ta=False, tb=True, K=40, aux=y,
                                ref=product64(A, B, False, True, precision) * elu_prime(y.double())))
    if nvil is not None:
        n_parts, B = nvil
        c["imp_parts"] = torch.rand(n_parts, B, generator=gen) * torch.tensor([2000.0, 300.0, 40.0, 5.0])[:n_parts, None] + 7.0
        c["baseline"] = torch.randn(B, generator=gen) * 10
        c["logp"] = -torch.rand(B, generator=gen) * 3
        c["ema"] = torch.tensor([800.0, 9.0, 0.9, 1.0])
    if n_kl:
        c["kl_parts"] = torch.rand(n_kl, M, generator=gen) * 5
    for k in ("dsample64", "loc", "scale"):
        assert bool(torch.isfinite(c[k]).all()), k
    return c


def gb_descs(c, base=1 << 20, extra=None):
    from attend_infer_repeat_amd import _lib
    mk = lambda ta, tb, M, N, K: _lib.AirGemmDesc(ta, tb, M, N, K, base, 4, base, 4, base, N, None, 0, None, 0, 0.0, None, c["precision"],
                                                  None, None, 0, None)
    descs = [mk(0, 1, c["M"], c["D"], c["K"])]
    if c.get("others"):
        descs = [mk(1, 0, 33, 20, 64), descs[0], mk(0, 1, 21, 70, 40)]
    if extra:
        descs.append(mk(1, 0, *extra))
    return descs


def sum_in_order32(parts):
    """float32 sum over the leading axis, taken in order from part 0 starting at 0.f (the loop of air_sum_leading / the share sums)"""
    s = torch.zeros_like(parts[0])
    for t in range(parts.shape[0]):
        s = s + parts[t]
    return s


# ---------------------------------------------------------------------------------------------------------------
# I. the feeder
# ---------------------------------------------------------------------------------------------------------------
FEED_SEED = 0x1234567890ABCDEF
# item_floats, B, n_items, step, shuffle
GATHER_CASES = [
    (2500, 5, 37, 0, True),             # vec4 rows
    (10, 5, 37, 3, True),               # item_floats % 4 != 0: the scalar copy
    (8, 4100, 37, 3, True),             # more rows than the 4096 workgroups: the grid-stride
    (8, 5, 1, 3, True),                 # one item: every index 0
    (1, 37, 2 ** 20 + 7, 3, True),      # an item count that is no power of two, indices beyond 2^20 (one float per item: 4 MB)
    (8, 5, 37, 2 ** 33, True),          # the 64-bit counter
    (8, 5, 37, 2 ** 33, False),         # sequential, 64-bit counter
    (2500, 37, 37, 3, False),           # sequential walk wrapping round the data
]


@functools.lru_cache(maxsize=None)
def gather_case(i):
    item_floats, B, n_items, step, shuffle = GATHER_CASES[i]
    idx = feeder_indices(FEED_SEED, step, B, n_items, shuffle)
    assert all(0 <= v < n_items for v in idx)
    data = torch.randn(n_items, item_floats, generator=torch.Generator().manual_seed(800 + i))
    return dict(item_floats=item_floats, B=B, n_items=n_items, step=step, shuffle=shuffle, idx=idx, data=data)


# B, the problems as (column offset, K, N, in copy_mask), idx_out given
GG_CASES = [
    (5, [(0, 2500, 50, True)], True),
    (37, [(0, 2500, 50, True)], False),
    (64, [(0, 2500, 256, True)], True),
    (5, [(0, 1288, 50, True), (1288, 1212, 20, True)], True),
    (37, [(0, 1288, 50, True), (1288, 1212, 20, True)], True),
    (64, [(0, 1288, 50, True), (1288, 1212, 20, True)], False),
    (37, [(0, 1288, 50, True), (1288, 1212, 20, True), (0, 1288, 33, False)], True),
    (64, [(0, 1288, 50, True), (1288, 1212, 20, True), (0, 1288, 33, False)], True),
    (37, [(0, 1288, 50, True), (1288, 1212, 20, False)], True),        # columns [1288, 2500) of obs in no problem of copy_mask: untouched
]
GG_ITEMS, GG_N_ITEMS, GG_STEP = 2500, 37, 3


@functools.lru_cache(maxsize=None)
def gg_case(i):
    B, probs, has_idx = GG_CASES[i]
    gen = torch.Generator().manual_seed(900 + i)
    data = torch.rand(GG_N_ITEMS, GG_ITEMS, generator=gen)
    idx = feeder_indices(FEED_SEED, GG_STEP, B, GG_N_ITEMS, True)
    obs = data[torch.tensor(idx)]
    c = dict(B=B, has_idx=has_idx, data=data, idx=idx, obs=obs, problems=[], copy_mask=0)
    cover = torch.zeros(GG_ITEMS, dtype=torch.int32)
    for j, (off, K, N, copy) in enumerate(probs):
        w = torch.randn(K, N, generator=gen) / K ** 0.5
        bias = torch.randn(N, generator=gen)
        c["problems"].append(dict(off=off, K=K, N=N, w=w, bias=bias, ref=obs[:, off:off + K].double() @ w.double() + bias.double()))
        assert off % 4 == 0
        if copy:
            c["copy_mask"] |= 1 << j
            cover[off:off + K] += 1
    assert bool((cover <= 1).all()), "the problems of copy_mask cover no column twice"
    assert sorted(p[1] & 15 for p in probs)[:2] in ([4], [8, 12], [8, 8])       # the masked last K chunk: 4, or 8 and 12 floats
    c["covered"] = cover == 1
    return c


def gg_descs(c, obs=1 << 20):
    """the case as AirGemmDesc records with A inside an obs buffer at byte address `obs` (for the host mirror of the fits rule)"""
    from attend_infer_repeat_amd import _lib
    return [_lib.AirGemmDesc(0, 0, c["B"], p["N"], p["K"], obs + 4 * p["off"], GG_ITEMS, 1 << 24, p["N"], 1 << 25, p["N"], 1 << 26, 1, None, 0,
                             0.0, None, 0, None, None, 0, None) for p in c["problems"]]


# what air_gemm_grouped_gather_fits says to one problem over obs[B, item_floats], changed in one respect at a time
FITS_BASE = dict(B=64, item_floats=2500, off=0, K=2500, N=64, ta=0, precision=0, M=None, lda=None, data_shift=0)
FITS_ACCEPTED = {
    "the base launch": dict(),
    "1000 tiles": dict(N=4000),                                                  # 4 * 250 tiles of 16 x 16: wide_min_tiles(), the last
    "K = 512 = 8 min(M, N)": dict(K=512, item_floats=512),
}
FITS_DECLINED = {
    "K = 508": dict(K=508, item_floats=508, N=16),
    "item_floats % 4 != 0": dict(item_floats=2502),
    "offset not a multiple of 4": dict(off=2, K=2496),
    "ta = 1": dict(ta=1),
    "bf16": dict(precision=1),
    "M != B": dict(M=48),
    "lda != item_floats": dict(lda=2504),
    "a misaligned dataset": dict(data_shift=4),
    "1025 tiles": dict(B=80, N=3280),                                            # 5 * 205 tiles, K = 2500 >= 8 * 80
    # more than wide_min_tiles() = 1000 tiles: air_gemm_grouped tests its wide-tile regime before the long-K split
    "1024 tiles: the wide-tile kernels": dict(N=4096),                           # 4 * 256 tiles; aligned, N and K multiples of 4
    "1004 tiles: the wide-tile kernels": dict(N=4004),                           # 4 * 251 tiles
    "off the long-K form: M = 128, N = 256, K = 512": dict(B=128, N=256, K=512, item_floats=512),
    "off the long-K form: M = N = 256, K = 1252": dict(B=256, N=256, K=1252, item_floats=1252),
}
# B, N, K of a lone NN product over the whole row, on either side of wide_min_tiles() = 1000 tiles, both ragged in M and with a masked
# last K chunk of 4 floats; N and K multiples of 4, so that only the tile count keeps the first off the wide-tile kernels.
# 4 * 250 = 1000 tiles: taken, and bit-equal to air_batch_gather + air_gemm_grouped (both on the 16-wave K split);
# 4 * 251 = 1004 tiles: declined (air_gemm_grouped runs it on gemm_wide_kernel)
GG_EDGE_TAKEN, GG_EDGE_DECLINED = (61, 3992, 516), (61, 4004, 516)


def fits_launch(change, obs=1 << 20, dataset=1 << 22):
    """FITS_BASE with `change` applied -> ([AirGemmDesc], dict(B, item_floats, dataset address)); the B operand and C are never read by
    the fits rule and sit at made-up addresses"""
    from attend_infer_repeat_amd import _lib
    f = dict(FITS_BASE, **change)
    M = f["B"] if f["M"] is None else f["M"]
    lda = f["item_floats"] if f["lda"] is None else f["lda"]
    d = _lib.AirGemmDesc(f["ta"], 0, M, f["N"], f["K"], obs + 4 * f["off"], lda, 1 << 24, f["N"], 1 << 25, f["N"], None, 0, None, 0, 0.0,
                         None, f["precision"], None, None, 0, None)
    return [d], dict(B=f["B"], item_floats=f["item_floats"], dataset=dataset + f["data_shift"], obs=obs)


# ---------------------------------------------------------------------------------------------------------------
# J. the step prologue and the first LSTM step
# ---------------------------------------------------------------------------------------------------------------
RNG_SEED, RNG_OFFSET = 0x0123456789ABCDEF, (1 << 32) - 3            # the counter crosses 2^32 inside the first quads
NOISE_SIZES = [(0, 7), (10, 0), (4097, 4099), (2_100_001, 3)]       # the last: more than 2048 x 256 quads, the noise loop strides
# The bound of test_observe_matches_rng_fill_numbers, |z - ref| <= 1e-6 (|ref| + 1), holds between two float32 evaluations of the same
# Box-Muller.  Against the float64 one it does not: the kernels form the angle 2 pi u2 as a float32 product (up to 2.4e-7 of rounding for
# an angle in [4, 8), plus 1.7e-7 u2 from the float32 value of 2 pi), and |d z| = rad |d th| where cos or sin is near 0, with rad up to
# 5.9.  Measured on the UNFUSED draw, air_rng_fill (the same quads; the prologue is bit-equal to it), over 2 100 001 normals against
# noise_ref: worst error / (1e-6 |ref| + 1e-6) = 1.373 at the state the tests use, 1.447 and 1.367 at two others (largest |z - ref|
# 1.7e-6).  One seed is a sample: twice the worst of the three, 2 x 1.447 = 2.894.
NORMAL_TOL = (2.894e-6, 2.894e-6)
PRIOR_TOL = (1e-12, 0.0)
TILE_SHAPES = [(5, 7), (37, 50), (1045, 128)]
LSTM_PRO_SHAPES = [(5, 7), (37, 50), (64, 256), (1045, 128)]        # the last: 528 tiles, the 512-thread wide kernel carries the prologue
# M, Hd, E, ldx, x offset by one float.  The launch takes a shape when (M, Hd) has at most 512 tiles AND the gx product [M, 4Hd, E] as a
# launch of its own runs on the 4-wave 16 x 16 body (at most 1000 tiles of gx, no long K): the body whose K order it repeats
FIRST_CASES = [
    (37, 50, 50, 52, False),            # vecX = 1: 16-byte rows
    (37, 50, 50, 52, True),             # the same rows starting one float in: vecX = 0
    (5, 16, 1, 1, False),               # E = 1
    (64, 256, 256, 256, False),         # the engine's own shape
    (5, 16, 50, 52, True),
    (400, 160, 52, 52, False),          # 25 * 40 = 1000 tiles of gx: the last shape the launch takes by that count
    (8192, 4, 4, 4, False),             # 512 tiles of (M, Hd) (and of gx): the last shape it takes by this one
]
# M, Hd, E, ldx: declined with AIR_E_UNSUPPORTED, nothing written
FIRST_DECLINED = {
    "513 tiles of (M, Hd)": (8208, 4, 4, 4),                                # (and 513 of gx: declined for this reason alone)
    "1040 tiles of gx: the wide-tile regime": (416, 160, 52, 52),           # 26 * 40 > 1000, E % 4 == 0
    "2048 tiles of gx: 32 x 32 tiles": (512, 256, 50, 52),                  # (512 tiles of (M, Hd): within the first limit)
    "2048 tiles of gx: the wide-tile kernels": (512, 256, 52, 52),          # where bf16 operands gave other bits than the two launches
    "a long K: the 16-wave split": (16, 16, 512, 512),                      # E = 512 >= 8 min(16, 64)
}


@functools.lru_cache(maxsize=None)
def lstm_case(M, Hd, E=None, ldx=None):
    gen = torch.Generator().manual_seed(M * 7 + Hd + (E or 0) * 1000)
    c = dict(M=M, Hd=Hd, E=E, ldx=ldx)
    c["h0"] = torch.randn(Hd, generator=gen) * 0.5; c["c0"] = torch.randn(Hd, generator=gen)
    rows = Hd + (E or 0)
    c["w_full"] = torch.randn(rows, 4 * Hd, generator=gen) / Hd ** 0.5        # [w_x ; w_h], like the engine's w_gates
    c["w_h"] = c["w_full"][rows - Hd:]
    if E is None:
        c["gx"] = torch.randn(M, 4 * Hd, generator=gen)
    else:
        c["w_x"] = c["w_full"][:E]
        c["x_buf"] = torch.randn(M, ldx, generator=gen)
        c["b"] = torch.randn(4 * Hd, generator=gen) * 0.3
    return c


def lstm_refs(c, precision):
    """gx64 (for the first step: x . w_x + b on the rounded operands) and the step on it -> gx64 | None, h64, c64, act64"""
    if c["E"] is None:
        gx64, gx = None, c["gx"]
    else:
        r = _rounded(precision)
        gx64 = r(c["x_buf"][:, :c["E"]]).double() @ r(c["w_x"]).double() + c["b"].double()
        gx = gx64
    h, cc, act = lstm64(c["h0"][None, :], c["c0"][None, :], c["w_h"], gx, 1.0, precision)
    return gx64, h, cc, act


# ---------------------------------------------------------------------------------------------------------------
# K. the small riders
# ---------------------------------------------------------------------------------------------------------------
CANVAS_SHAPES = [(3, 5, 17, 13, 5, 7), (2, 70, 28, 36, 9, 12)]
CANVAS_MULT, CANVAS_STD = 0.5, 0.3


@functools.lru_cache(maxsize=None)
def canvas_case(i):
    T, B, H, W, h, w = CANVAS_SHAPES[i]
    rng = np.random.default_rng(70 + i)
    c = dict(T=T, B=B, H=H, W=W, h=h, w=w)
    c["glimpse"] = torch.as_tensor(rng.standard_normal((T, B, h, w)).astype(np.float32))
    c["where"] = torch.as_tensor(rand_where(T * B, rng).reshape(T, B, 4))
    c["presence"] = torch.as_tensor(rng.uniform(0.2, 1.0, (T, B)).astype(np.float32))         # continuous steps
    c["obs"] = torch.as_tensor(rng.random((B, H, W)).astype(np.float32))
    c["loss_scale"] = 1.0 / B
    tp = c["presence"].double().requires_grad_(True)
    tg, tw = c["glimpse"].double(), c["where"].double()
    cv = sum(tp[t][:, None, None] * O.st_write(tg[t], tw[t], (H, W)) for t in range(T))
    nll = 0.5 * ((c["obs"].double() - CANVAS_MULT * cv) / CANVAS_STD) ** 2 + 0.5 * np.log(2 * np.pi) + np.log(CANVAS_STD)
    c["dpresence64"], = torch.autograd.grad(nll.sum((1, 2)).sum() * f32v(c["loss_scale"]), [tp])
    assert bool(torch.isfinite(c["dpresence64"]).all())
    return c


DPRESENCE_TOL = (2e-4, 2e-5)                                          # what test_st_write_bwd holds dwhere to (scaled the same way)
SUM_LEADING = [(T, n) for T in (1, 4, 7) for n in (1, 255, 4099)]
