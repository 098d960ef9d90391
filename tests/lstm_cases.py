"""Case builders and float64 references for the kernel-level tests of the LSTM recurrence (tests/test_lstm_kernels.py): the forward
steps with a full h_prev (air_lstm_step_fwd, air_lstm_step_fwd_bf16, air_lstm_pointwise_fwd), one BPTT link (air_lstm_step_bwd[_opt],
air_lstm_step_bwd_bf16, air_lstm_pointwise_bwd[_bf16]), the entry of the BPTT folded into its first link (air_lstm_step_bwd_entry) and
whole chains wired as engine_plan._PlanBuilder.bptt wires them.  Importable without a GPU; tests/test_lstm_cases_host.py builds every
case on the CPU, holds it against the host mirrors of the dispatch rules (attend_infer_repeat_amd/gemm_groups.py) and checks the
references against torch.autograd.  No test lives here.

Every builder is cached and returns float32 inputs with float64 expectations as CPU tensors.  Two input regimes:
  * "unit": the distributions of tests/test_hip_kernels.py (randn operands, weights randn / sqrt(Hd), gate activations that a
    forward step produced);
  * "planted": values drawn from the short lists below -- saturated gates (expf(-x) overflowing inside sigmoid_acc, gate values of
    exactly 0 and 1), cell states on the tanh plateau, where 1 - tc * tc cancels.  Every list value occurs at least once per tensor;
    that is asserted where the tensor is made.
Every reference is asserted finite."""
import functools

import torch

from attend_cases import SENTINEL, WORST, _rounded, assert_bits, assert_close, g, print_worst  # noqa: F401
from fold_cases import BF16, F32, LSTM_TOL, RMS_TOL, lstm64, rmsprop64  # noqa: F401

from attend_infer_repeat_amd import gemm_groups as G

# The bounds are the project's own: LSTM_TOL (fold_cases.py) for h, c, gate_act; for the backward what
# test_lstm_fused_step_matches_unfused_pair_and_fp64 holds dgates / dc_prev / dgx to; against the unfused pair 1e-5 where the K order
# differs (same test); the entry against its two launches as test_lstm_bwd_entry_matches_pointwise_plus_link_and_fp64: 1e-6 for the
# results of step T-1, 1e-5 for those of the link.
BWD_TOL = (1e-4, 2e-5)
PAIR_TOL = (1e-5, 1e-5)
ENTRY_PAIR_TOL_LAST, ENTRY_PAIR_TOL_LINK = (1e-6, 1e-6), (1e-5, 1e-5)
# The entry evaluates tanh(c) as 1 - 2 / (exp(2 c) + 1) (absolute error about 1e-7), the pointwise launch with libm's tanhf.  With unit
# cell states the two agree within 1e-6; a planted c_prev1 of 60 multiplies the difference of 1 - tc * tc by |c_prev1| gf (1 - gf) = 15
# on its way into the forget gate's dgates1.  The plain float32 restatement of the two forms on the CPU (entry_last32: correctly
# rounded exp and division against torch.tanh) differs by r = 2.139 of 1e-6 |ref| + 1e-6 at (64, 512) "all" (1.959 at (512, 256), 1.571
# at (64, 256), 1.397 at (37, 48); dc_prev1 0.22 at most; unit regime 0.59 at most), so on planted cell states dgates1 is held to 8 r
# = 17.11 of that bound -- the factor for the fast intrinsics (__expf, __fdividef) of the kernel.  On the GPU the comparison measured
# 2.34 of the borrowed bound at (512, 256).  Unit cell states and dc_prev1 keep 1e-6.
ENTRY_FAST_TANH_R = 2.139
ENTRY_PAIR_TOL_LAST_PLANTED = (8 * ENTRY_FAST_TANH_R * 1e-6, 8 * ENTRY_FAST_TANH_R * 1e-6)
RESTATEMENT_SHARE = 0.25            # the float32 restatement of every comparison stays within this share of its bound (host test)

GX_LIST = [0.0, 1e-3, -1e-3, 4.0, -4.0, 17.0, -17.0, 40.0, -40.0, 90.0, -90.0]
C_LIST = [0.0, 1e-4, -1e-4, 0.5, -0.5, 3.0, -3.0, 9.0, -9.0, 30.0, -30.0, 44.0, -44.0, 60.0, -60.0]
GATE_LIST = [0.0, 1e-7, 0.25, 0.5, 1.0 - 2.0 ** -24, 1.0]
FORGET_BIASES = (1.0, 0.0, -2.5)
UNIT, PLANTED = "unit", "planted"
# The scale of the gradient that enters a link's product (dgates_next; for the entry the dh terms of step T-1, from which it forms that
# operand).  Unit: 0.3, as test_lstm_fused_step_matches_unfused_pair_and_fp64.  Planted: a planted c_prev multiplies every rounding
# error of the product by up to |c_prev| gf (1 - gf) = 60 / 4 on its way into dgates, while the absolute part of BWD_TOL was set for
# unit-scale cell states; at 0.3 the plain float32 restatement of the link alone spent 0.26 of the bound at (512, 256) and 0.42 in the
# entry at (64, 512) (K = 2048), past the quarter it may spend, so the planted gradients enter at a third of that.
GRAD_SCALE = {UNIT: 0.3, PLANTED: 0.1}


def planted(gen, shape, values, signs=False):
    """a float32 tensor drawn from `values` in which every value occurs (signs: each entry negated with probability 1/2, every value
    in both signs)"""
    v = torch.tensor(values, dtype=torch.float32)
    if signs:
        v = torch.cat([v, -v])
    n = 1
    for s in shape:
        n *= s
    assert n >= len(v), "a tensor too small to hold every planted value"
    idx = torch.randint(len(v), (n,), generator=gen)
    idx[torch.randperm(n, generator=gen)[:len(v)]] = torch.arange(len(v))
    out = v[idx].reshape(shape)
    for x in v.tolist():
        assert bool((out == x).any()), f"planted value {x} missing"
    assert float(out.max()) == float(v.max()) and float(out.min()) == float(v.min())
    return out


def _finite(c, keys):
    for k in keys:
        assert bool(torch.isfinite(c[k]).all()), k
    return c


def _seed(*v):
    s = 17
    for x in v:
        s = (s * 1000003 + (hash(x) if not isinstance(x, str) else sum(ord(ch) for ch in x))) % (2 ** 31)
    return s


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def lstm_fwd_ref(h_prev, c_prev, w_h, gx, forget_bias, precision, dtype=torch.float64):
    """fold_cases.lstm64 with the arithmetic in `dtype` (float32: the restatement the host test measures); at float64 it IS lstm64"""
    r = _rounded(precision)
    pre = r(h_prev).to(dtype) @ r(w_h).to(dtype) + gx.to(dtype)
    i, j, f, o = torch.chunk(pre, 4, -1)
    gi, gj, gf, go = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + forget_bias), torch.sigmoid(o)
    c = gf * c_prev.to(dtype) + gi * gj
    return torch.tanh(c) * go, c, torch.cat([gi, gj, gf, go], -1)


def lstm_bwd64(dgates_next, w_h, dh_a, dh_b, dc_in, gate_act, c_prev, c, dgx_in=None, precision=F32, dtype=torch.float64):
    """One BPTT link in float64: dh = dgates_next . w_h^T + dh_a + dh_b (operands of the product rounded to bf16 first for precision
    1), then the gate backward on the float32 gate_act, c_prev, c handed to the kernel.  Any optional term may be None; without
    dgates_next there is no product (the pointwise backward of the last step).  -> dgates, dc_prev, dgx = dgx_in + dgates"""
    r = _rounded(precision)
    a = gate_act.to(dtype)
    dh = torch.zeros_like(c_prev, dtype=dtype)
    if dgates_next is not None:
        dh = r(dgates_next).to(dtype) @ r(w_h).to(dtype).t()
    for t in (dh_a, dh_b):                                      # (v + dh_a) + dh_b: the order of the kernels
        if t is not None:
            dh = dh + t.to(dtype)
    gi, gj, gf, go = torch.chunk(a, 4, -1)
    tc = torch.tanh(c.to(dtype))
    dct = dh * go * (1 - tc * tc)
    if dc_in is not None:
        dct = dc_in.to(dtype) + dct
    d = torch.cat([dct * gj * gi * (1 - gi), dct * gi * (1 - gj * gj), dct * c_prev.to(dtype) * gf * (1 - gf), dh * tc * go * (1 - go)], -1)
    return d, dct * gf, d if dgx_in is None else dgx_in.to(dtype) + d


def chain64(h0, c0, w_h, gx, T, dH, dH_b, forget_bias=1.0, dtype=torch.float64):
    """The free-running recurrence of T steps from one broadcast h0 / c0 row [Hd] and a fixed gx [M, 4Hd], and its backward with the
    direct terms dH[t], dH_b[t] [M, Hd] of every step (either may be None).  -> dict: h_seq, c_seq [T+1, M, Hd] (index 0: the tiled
    initial state), gate_act, dgates [T, M, 4Hd], dgx_after [T, M, 4Hd] (the running sum as it stands once step t is done: index T-1
    is dgates[T-1], index 0 the final dgx), dc0 [M, Hd]"""
    M = gx.shape[0]
    h, c = h0.to(dtype)[None, :].expand(M, -1), c0.to(dtype)[None, :].expand(M, -1)
    hs, cs, acts = [h], [c], []
    for t in range(T):
        h, c, act = lstm_fwd_ref(h, c, w_h, gx, forget_bias, F32, dtype)
        hs.append(h); cs.append(c); acts.append(act)
    dg, run, dgn, dc, dgx = [None] * T, [None] * T, None, None, None
    for t in reversed(range(T)):
        d, dc, dgx = lstm_bwd64(dgn, w_h, None if dH is None else dH[t], None if dH_b is None else dH_b[t], dc, acts[t], cs[t], cs[t + 1],
                                dgx, F32, dtype)
        dg[t], run[t], dgn = d, dgx, d
    return dict(h_seq=torch.stack(hs), c_seq=torch.stack(cs), gate_act=torch.stack(acts), dgates=torch.stack(dg), dgx_after=torch.stack(run),
                dc0=dc)


def ratio(got, ref, tol):
    """worst |got - ref| / (atol + rtol |ref|)"""
    rtol, atol = tol
    ref = ref.double()
    return float(((got.double() - ref).abs() / (atol + rtol * ref.abs())).max())


# ---------------------------------------------------------------------------------------------------------------
# L. forward steps with a full h_prev
# ---------------------------------------------------------------------------------------------------------------
# M, Hd, layout, the body lstm_fwd_launch gives it.  layout "h_off": h_prev based 4 bytes off a 16-byte boundary; "ldw3": w_h a view of
# leading dimension 4 Hd + 3 -- either keeps a launch of more than 512 tiles off the wide kernel
FWD_SHAPES = [
    (5, 7, "", "fused"),                # K tail only (Hd < 16); Hd % 4 != 0: ldh % 4 != 0, vecA = 0; column-edge tiles
    (37, 50, "", "fused"),              # K tail of 2; vecA = 0
    (130, 40, "", "fused"),             # vecA = 1; K tail of 8
    (64, 256, "", "fused"),             # the engine's own shape
    (512, 256, "", "fused"),            # 32 * 16 = 512 tiles: the last fused launch
    (2048, 64, "", "fused"),            # 128 * 4 = 512 tiles: the last fused launch
    (513, 256, "", "wide"),             # 528 tiles; one valid row in the last row tile
    (2049, 64, "", "wide"),             # 516 tiles; four K chunks for eight waves
    (513, 256, "h_off", "fused"),       # 528 tiles on the 4-wave body: h_prev misaligned
    (513, 256, "ldw3", "fused"),        # 528 tiles on the 4-wave body: ldw % 4 != 0
    (2049, 50, "", "fused"),            # 516 tiles, Hd % 64 != 0
]


def _fwd_variants(s):
    """every shape with ldgx = 4 Hd + 8 and + 3, in both regimes and precisions; the three forget biases go round the table"""
    alt = (0.0, -2.5)
    return [(8, UNIT, 1.0, F32), (3, PLANTED, alt[s % 2], F32), (8, PLANTED, 1.0, BF16), (3, UNIT, alt[(s + 1) % 2], BF16)]


# (M, Hd, layout, body, ldgx - 4 Hd, regime, forget_bias, precision)
FWD_RUNS = [sh + v for s, sh in enumerate(FWD_SHAPES) for v in _fwd_variants(s)]
# air_lstm_pointwise_fwd: (M, Hd, regime, forget_bias, gate_act given).  (2049, 256): 524 544 elements, more than the 2048 x 256 threads
# of the largest grid -- the only shape at which the element loop goes round
PW_FWD_RUNS = [(5, 7, UNIT, 1.0, True), (37, 50, PLANTED, 0.0, True), (37, 50, PLANTED, -2.5, False), (2049, 256, UNIT, 1.0, True),
               (2049, 256, PLANTED, 1.0, False)]
# air_lstm_step_fwd_bf16 / _bwd_bf16 / air_lstm_pointwise_bwd_bf16: (M, Hd, input mirrors given, regime)
BF16MEM_RUNS = [(513, 256, False, UNIT), (513, 256, True, PLANTED), (2049, 64, False, PLANTED), (2049, 64, True, UNIT), (48, 64, False, UNIT),
                (48, 64, True, PLANTED)]
BASE = 1 << 20                                                  # a made-up 16-byte aligned address for the host mirrors


def fwd_body(M, Hd, layout):
    wide = G.lstm_fwd_wide(M, Hd, ldw=4 * Hd + (3 if layout == "ldw3" else 0), ldh=Hd, w_h=BASE, h_prev=BASE + (4 if layout == "h_off" else 0))
    return "wide" if wide else "fused"


def fwd_pair_is_bitwise(M, Hd, layout):
    """the step repeats the K order of the 4-wave 16 x 16 body: bit-equal to product + pointwise where the step runs on its 4-wave
    kernel and air_gemm_grouped runs the product [M, 4 Hd, Hd] alone on that body"""
    return fwd_body(M, Hd, layout) == "fused" and G.lone_on_tile16_kw4(M, 4 * Hd, Hd)


@functools.lru_cache(maxsize=None)
def fwd_case(M, Hd, regime, precision, forget_bias):
    gen = torch.Generator().manual_seed(_seed("fwd", M, Hd, regime))
    c = dict(M=M, Hd=Hd, regime=regime, precision=precision, fb=forget_bias)
    c["h_prev"] = torch.randn(M, Hd, generator=gen) * 0.5
    c["w_h"] = torch.randn(Hd, 4 * Hd, generator=gen) / Hd ** 0.5
    if regime == UNIT:
        c["c_prev"] = torch.randn(M, Hd, generator=gen)
        c["gx"] = torch.randn(M, 4 * Hd, generator=gen)
    else:
        c["c_prev"] = planted(gen, (M, Hd), C_LIST)
        c["gx"] = planted(gen, (M, 4 * Hd), GX_LIST)
    c["h64"], c["c64"], c["act64"] = lstm64(c["h_prev"], c["c_prev"], c["w_h"], c["gx"], forget_bias, precision)
    return _finite(c, ("h64", "c64", "act64"))


# ---------------------------------------------------------------------------------------------------------------
# M. one BPTT link
# ---------------------------------------------------------------------------------------------------------------
# M, Hd, layout, the body lstm_bwd_launch gives it.  layout "dgn_off" / "w_off": dgates_next / w_h based 4 bytes off
BWD_SHAPES = [
    (5, 7, "", "kw16"),
    (37, 50, "", "kw16"),               # K = 200: a tail of 8 for wave 12
    (130, 40, "", "kw16"),
    (64, 256, "", "kw16"),
    (512, 256, "", "kw16"),             # 512 tiles: the last 16-wave launch
    (2048, 64, "", "kw16"),
    (513, 256, "", "wide"),
    (2049, 64, "", "wide"),
    (513, 256, "dgn_off", "kw4"),
    (513, 256, "w_off", "kw4"),
    (2049, 50, "", "kw4"),
]
# (M, Hd, layout, body, regime, precision): every shape in both regimes and precisions
BWD_RUNS = [sh + v for sh in BWD_SHAPES for v in ((UNIT, F32), (PLANTED, F32), (UNIT, BF16), (PLANTED, BF16))]
# the optional operands of a link: name -> (dh_a, dh_b, dc_in given; dgx_in: None | "own" | "inplace" | "next"; dgx_out given)
PATTERNS = {
    "all": (True, True, True, "own", True),
    "none": (False, False, False, None, False),
    "dh_b": (False, True, False, None, False),
    "dgx_out": (True, False, True, None, True),              # dgx_out without dgx_in: dgx = dgates
    "inplace": (True, True, True, "inplace", True),          # dgx_in == dgx_out: the engine's wiring below t = T-2
    "acc_next": (True, True, True, "next", True),            # dgx_in = dgates_next: the engine's wiring at t = T-2
}
# air_lstm_pointwise_bwd with dh2, and its _bf16 form: (M, Hd, regime)
PW_BWD_RUNS = [(5, 7, UNIT), (37, 50, PLANTED), (2049, 256, UNIT)]


def bwd_body(M, Hd, layout):
    return G.lstm_bwd_form(M, Hd, dgates_next=BASE + (4 if layout == "dgn_off" else 0), w_h=BASE + (4 if layout == "w_off" else 0))


def bwd_pair_is_bitwise(M, Hd, layout):
    """the link repeats the K order of the body with its wave count: bit-equal to the product [M, Hd, 4 Hd] (beta = 1) + the pointwise
    backward where air_gemm_grouped runs that product alone on the 16-wave K split (link on 16 waves) or on the 4-wave 16 x 16 body
    (link on 4 waves)"""
    body = bwd_body(M, Hd, layout)
    if body == "kw16":
        return G.long_k(M, Hd, 4 * Hd) and ((M + 15) // 16) * ((Hd + 15) // 16) <= 1000
    return body == "kw4" and G.lone_on_tile16_kw4(M, Hd, 4 * Hd)


def _planted_act(gen, M, Hd):
    """gate activations from GATE_LIST: every value among the i / f / o columns, every value in both signs among the j columns"""
    ifo = planted(gen, (M, 3 * Hd), GATE_LIST)
    return torch.cat([ifo[:, :Hd], planted(gen, (M, Hd), GATE_LIST, signs=True), ifo[:, Hd:]], 1)


def _saved_state(gen, M, Hd, regime):
    """gate_act, c_prev, c of a step as float32: what a forward step wrote (unit: the float64 step, rounded), or planted"""
    if regime == UNIT:
        f = fwd_case(M, Hd, UNIT, F32, 1.0)
        return f["act64"].float(), f["c_prev"], f["c64"].float()
    return _planted_act(gen, M, Hd), planted(gen, (M, Hd), C_LIST), planted(gen, (M, Hd), C_LIST)


@functools.lru_cache(maxsize=None)
def bwd_case(M, Hd, regime):
    gen = torch.Generator().manual_seed(_seed("bwd", M, Hd, regime))
    c = dict(M=M, Hd=Hd, regime=regime)
    c["gate_act"], c["c_prev"], c["c"] = _saved_state(gen, M, Hd, regime)
    c["w_h"] = fwd_case(M, Hd, UNIT, F32, 1.0)["w_h"]
    c["dgates_next"] = torch.randn(M, 4 * Hd, generator=gen) * GRAD_SCALE[regime]
    for k in ("dh_a", "dh_b", "dc_in"):
        c[k] = torch.randn(M, Hd, generator=gen)
    c["dgx_in"] = torch.randn(M, 4 * Hd, generator=gen)
    return c


def pattern_operands(c, pattern):
    """the operands of PATTERNS[pattern] as CPU tensors | None: dh_a, dh_b, dc_in, dgx_in"""
    a, b, dc, dgx_in, _ = PATTERNS[pattern]
    src = {None: None, "own": c["dgx_in"], "inplace": c["dgx_in"], "next": c["dgates_next"]}[dgx_in]
    return c["dh_a"] if a else None, c["dh_b"] if b else None, c["dc_in"] if dc else None, src


@functools.lru_cache(maxsize=None)
def bwd_ref(M, Hd, regime, precision, pattern, dtype=torch.float64):
    c = bwd_case(M, Hd, regime)
    dh_a, dh_b, dc_in, dgx_in = pattern_operands(c, pattern)
    out = lstm_bwd64(c["dgates_next"], c["w_h"], dh_a, dh_b, dc_in, c["gate_act"], c["c_prev"], c["c"], dgx_in, precision, dtype)
    for t in out:
        assert bool(torch.isfinite(t).all())
    return out


# ---------------------------------------------------------------------------------------------------------------
# N. air_lstm_step_bwd_entry
# ---------------------------------------------------------------------------------------------------------------
# (5, 16): one unit chunk for sixteen waves; (64, 512): two rounds of unit chunks; (512, 256): 512 tiles, the last that fits
ENTRY_SHAPES = [(5, 16), (37, 48), (64, 256), (64, 512), (512, 256)]
ENTRY_RUNS = [(M, Hd, regime) for M, Hd in ENTRY_SHAPES for regime in (UNIT, PLANTED)]
# air_lstm_step_bwd_entry_fits, derived by hand: tiles = ceil(M / 16) * Hd / 16
ENTRY_FITS_TABLE = [(512, 256, True), (513, 256, False), (8192, 16, True), (8193, 16, False), (2048, 64, True), (2049, 64, False),
                    (16, 8192, True), (16, 8208, False), (17, 8192, False), (64, 250, False), (64, 8, False), (0, 16, False), (16, 0, False)]
ENTRY_VARIANTS = ["all", "no dh_a1", "no dh_b1", "no dgx_out"]


@functools.lru_cache(maxsize=None)
def entry_case(M, Hd, regime):
    """step T-1 (gate_act1, c_prev1 = c1, c of it = c2, dh_a1, dh_b1) and step T-2 (gate_act, c_prev = c0, c = c1, dh_a, dh_b)"""
    gen = torch.Generator().manual_seed(_seed("entry", M, Hd, regime))
    rn = lambda *s: torch.randn(*s, generator=gen)
    c = dict(M=M, Hd=Hd, regime=regime, w_h=rn(Hd, 4 * Hd) / Hd ** 0.5)
    if regime == UNIT:
        for k in ("act1", "act0"):
            c[k] = torch.sigmoid(rn(M, 4 * Hd)); c[k][:, Hd:2 * Hd] = torch.tanh(rn(M, Hd))
        c["c0"], c["c1"], c["c2"] = rn(M, Hd), rn(M, Hd), rn(M, Hd)
    else:
        for k in ("act1", "act0"):
            c[k] = _planted_act(gen, M, Hd)
        c["c0"], c["c1"], c["c2"] = (planted(gen, (M, Hd), C_LIST) for _ in range(3))
    for k in ("dh_a1", "dh_b1", "dh_a0", "dh_b0"):
        c[k] = rn(M, Hd)
    if regime == PLANTED:                                         # (they form the A operand of the link's product: see GRAD_SCALE)
        c["dh_a1"] *= GRAD_SCALE[PLANTED] / GRAD_SCALE[UNIT]; c["dh_b1"] *= GRAD_SCALE[PLANTED] / GRAD_SCALE[UNIT]
    return c


def entry_ref(c, variant="all", dtype=torch.float64):
    """-> dgates1, dc_prev1, dgates, dc_prev, dgx | None: two links of lstm_bwd64, free-running in `dtype`"""
    a1 = None if variant == "no dh_a1" else c["dh_a1"]
    b1 = None if variant == "no dh_b1" else c["dh_b1"]
    d1, dcp1, _ = lstm_bwd64(None, None, a1, b1, None, c["act1"], c["c1"], c["c2"], None, F32, dtype)
    d0, dcp0, dgx = lstm_bwd64(d1, c["w_h"], c["dh_a0"], c["dh_b0"], dcp1, c["act0"], c["c0"], c["c1"], d1, F32, dtype)
    out = (d1, dcp1, d0, dcp0, None if variant == "no dgx_out" else dgx)
    for t in out:
        assert t is None or bool(torch.isfinite(t).all())
    return out


def entry_last32(c, variant, fast):
    """dgates1, dc_prev1 in plain float32 with tanh(c) in the entry's form (fast) or as torch.tanh: the restatement of the comparison
    between the entry and air_lstm_pointwise_bwd"""
    a1 = None if variant == "no dh_a1" else c["dh_a1"]
    b1 = None if variant == "no dh_b1" else c["dh_b1"]
    gi, gj, gf, go = torch.chunk(c["act1"], 4, -1)
    tc = 1 - 2 / (torch.exp(2 * c["c2"]) + 1) if fast else torch.tanh(c["c2"])
    dhe = (0 if a1 is None else a1) + (0 if b1 is None else b1)
    dct = dhe * go * (1 - tc * tc)
    return torch.cat([dct * gj * gi * (1 - gi), dct * gi * (1 - gj * gj), dct * c["c1"] * gf * (1 - gf), dhe * tc * go * (1 - go)], -1), dct * gf


# ---------------------------------------------------------------------------------------------------------------
# O. chains
# ---------------------------------------------------------------------------------------------------------------
# (M, Hd, T); the entry fold where it fits and T >= 2, as _PlanBuilder.bptt decides
CHAIN_RUNS = [(21, 48, T) for T in (1, 2, 3, 8)] + [(64, 256, T) for T in (1, 2, 3, 8)] + [(2049, 64, 3), (2049, 50, 2)]
# precision = 1 and the _bf16 entries, step by step on what the previous launch wrote: (M, Hd, T, the _bf16 entries with mirrors)
CHAIN16_RUNS = [(21, 48, 3, False), (64, 256, 3, False), (64, 256, 3, True), (2049, 64, 3, False), (2049, 64, 3, True), (2049, 50, 2, False)]


def chain_uses_entry(M, Hd, T):
    return T >= 2 and G.lstm_bwd_entry_fits(M, Hd)


@functools.lru_cache(maxsize=None)
def chain_case(M, Hd, T):
    gen = torch.Generator().manual_seed(_seed("chain", M, Hd, T))
    c = dict(M=M, Hd=Hd, T=T)
    c["h0"] = torch.randn(Hd, generator=gen) * 0.5; c["c0"] = torch.randn(Hd, generator=gen)
    c["w_h"] = torch.randn(Hd, 4 * Hd, generator=gen) / Hd ** 0.5           # (doubled recurrent weights leave the float32 restatement's share)
    c["gx"] = torch.randn(M, 4 * Hd, generator=gen)
    c["dH"] = torch.randn(T, M, Hd, generator=gen); c["dH_b"] = torch.randn(T, M, Hd, generator=gen)
    c["ref"] = chain64(c["h0"], c["c0"], c["w_h"], c["gx"], T, c["dH"], c["dH_b"])
    _finite(c["ref"], tuple(c["ref"]))
    return c


# ---------------------------------------------------------------------------------------------------------------
# Q. an optimiser slice riding on a link
# ---------------------------------------------------------------------------------------------------------------
RIDER_SHAPE = (2049, 50, "", "kw4")
RIDER_RUNS = [RIDER_SHAPE]                  # the only case behind (air_lstm_step_bwd_opt, lstm_bwd_fused_kernel<4>)
RIDER_N, RIDER_LO, RIDER_HI = 8192, 1024, 6140
RIDER_HYPER = dict(lr=1e-3, decay=0.9, momentum=0.9, eps=1e-10)


@functools.lru_cache(maxsize=None)
def rider_case():
    gen = torch.Generator().manual_seed(4242)
    n = RIDER_N
    c = dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen), mg=torch.randn(n, generator=gen) * 0.5,
             mom=torch.randn(n, generator=gen) * 0.01)
    c["ms"] = (c["mg"].double() ** 2 + 0.2 + torch.rand(n, generator=gen).double()).float()
    assert bool((c["ms"].double() - c["mg"].double() ** 2 >= 0.1).all())
    assert RIDER_LO % 4 == 0 and RIDER_HI % 4 == 0 and 0 < RIDER_LO < RIDER_HI < n
    lo, hi = RIDER_LO, RIDER_HI
    c["ref"] = rmsprop64(c["p"][lo:hi], c["g"][lo:hi], c["ms"][lo:hi], c["mg"][lo:hi], c["mom"][lo:hi], float(torch.tensor(RIDER_HYPER["lr"])),
                         RIDER_HYPER["decay"], RIDER_HYPER["momentum"], RIDER_HYPER["eps"], 1.0)
    return c


# ---------------------------------------------------------------------------------------------------------------
# what the cases reach: (entry, kernel body, precision) -- tests/test_lstm_cases_host.py fails if a row of DECLARED is reached by none
# ---------------------------------------------------------------------------------------------------------------
DECLARED = {
    ("air_lstm_step_fwd", "lstm_fwd_fused_kernel", F32), ("air_lstm_step_fwd", "lstm_fwd_fused_kernel", BF16),
    ("air_lstm_step_fwd", "lstm_fwd_wide_kernel", F32), ("air_lstm_step_fwd", "lstm_fwd_wide_kernel", BF16),
    ("air_lstm_step_fwd_bf16", "lstm_fwd_wide16_kernel", BF16),
    ("air_lstm_pointwise_fwd", "lstm_pw_fwd_kernel", F32),
    ("air_lstm_step_bwd", "lstm_bwd_fused_kernel<16>", F32), ("air_lstm_step_bwd", "lstm_bwd_fused_kernel<16>", BF16),
    ("air_lstm_step_bwd", "lstm_bwd_fused_kernel<4>", F32), ("air_lstm_step_bwd", "lstm_bwd_fused_kernel<4>", BF16),
    ("air_lstm_step_bwd", "lstm_bwd_wide_kernel", F32), ("air_lstm_step_bwd", "lstm_bwd_wide_kernel", BF16),
    ("air_lstm_step_bwd_opt", "lstm_bwd_fused_kernel<4>", F32),
    ("air_lstm_step_bwd_bf16", "lstm_bwd_wide16_kernel", BF16),
    ("air_lstm_step_bwd_entry", "lstm_bwd_entry_kernel", F32),
    ("air_lstm_pointwise_bwd", "lstm_pw_bwd_kernel", F32),
    ("air_lstm_pointwise_bwd_bf16", "lstm_pw_bwd_mirror_kernel", BF16),
    ("air_lstm_pointwise_bwd_opt", "lstm_pw_bwd_opt_kernel", F32),
}
_FWD_KERNEL = {"fused": "lstm_fwd_fused_kernel", "wide": "lstm_fwd_wide_kernel"}
_BWD_KERNEL = {"kw16": "lstm_bwd_fused_kernel<16>", "kw4": "lstm_bwd_fused_kernel<4>", "wide": "lstm_bwd_wide_kernel"}


def reached():
    """{(entry, body, precision): [the runs that reach it]} by the host mirrors of the dispatch rules"""
    out = {}
    add = lambda key, run: out.setdefault(key, []).append(run)
    for run in FWD_RUNS:
        M, Hd, layout, _, _, _, _, precision = run
        add(("air_lstm_step_fwd", _FWD_KERNEL[fwd_body(M, Hd, layout)], precision), ("L", run))
    for run in PW_FWD_RUNS:
        add(("air_lstm_pointwise_fwd", "lstm_pw_fwd_kernel", F32), ("L", run))
    for run in BF16MEM_RUNS:
        assert G.lstm_bf16_fits(run[0], run[1])
        add(("air_lstm_step_fwd_bf16", "lstm_fwd_wide16_kernel", BF16), ("L", run))
        add(("air_lstm_step_bwd_bf16", "lstm_bwd_wide16_kernel", BF16), ("M", run))
        add(("air_lstm_pointwise_bwd_bf16", "lstm_pw_bwd_mirror_kernel", BF16), ("M", run))
    for run in BWD_RUNS:
        M, Hd, layout, _, _, precision = run
        add(("air_lstm_step_bwd", _BWD_KERNEL[bwd_body(M, Hd, layout)], precision), ("M", run))
    for run in PW_BWD_RUNS:
        add(("air_lstm_pointwise_bwd", "lstm_pw_bwd_kernel", F32), ("M", run))
    for run in ENTRY_RUNS:
        if G.lstm_bwd_entry_fits(run[0], run[1]):
            add(("air_lstm_step_bwd_entry", "lstm_bwd_entry_kernel", F32), ("N", run))
    for run in RIDER_RUNS:
        M, Hd, layout, _ = run
        add(("air_lstm_step_bwd_opt", _BWD_KERNEL[bwd_body(M, Hd, layout)], F32), ("Q", run))
    add(("air_lstm_pointwise_bwd_opt", "lstm_pw_bwd_opt_kernel", F32), ("Q", PW_BWD_RUNS[1]))
    return out
