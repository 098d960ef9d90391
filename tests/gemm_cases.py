"""Case table, builders, float64 references, bounds and float32 restatements for the kernel-level tests of the GEMM family
(tests/test_gemm_kernels.py): air_gemm, air_gemm_bf16, air_linear_fwd / air_linear_bwd and air_gemm_grouped on every kernel its launch
switch can reach -- gemm_body <1,1,4> / <1,1,16> / <2,2,4> / <2,2,1> with the split-K epilogue kernel, the c16 and A-prologue forms, the
short-K streaming body, gemm_wide_body, gemm_wide16_body with its four mirror combinations and the big-group kernels.  Importable
without a GPU; tests/test_gemm_cases_host.py holds every row of the table against the host mirror of the dispatch
(attend_infer_repeat_amd/gemm_groups.py grouped_form / single_form) and against the library's own queries (air_gemm_grouped_form /
air_gemm_form), checks that every reachable kernel has a row, and sets the bound's constants.  No test lives here.

Inputs.  Every operand element has a magnitude uniform in [0.5, 1.5] and a random sign: a single product term is at least 0.25, so a
dropped term cannot hide.  Every operand, aux, bias and C-for-beta is a view into a NaN-filled flat parent: at least two NaN rows in
front, NaN columns behind each row where ld > cols, NaN rows behind.  The view starts at `lead` floats into a parent whose base is
aligned far beyond 16 bytes, so lead % 4 decides the 16-byte alignment the dispatch tests (a_un / b_un: one float further).

References are float64: the product of the operands (rounded to bf16 first in precision 1), the epilogue in float64, colsum as the
float64 sum of the UNROUNDED fp32 B.

The bound is elementwise and a function of float64 quantities of the case only:
    |out - out64| <= CONST[group] * 2^-24 * (S + |beta C0| + |bias| + |aux| + [ELU: 1] + |out64|),   S = sum_k |a_mk b_kn|
(the terms have random signs, so the partial sums of a chain stay near S / sqrt(K) and its K roundings, each half a unit of such a
partial sum, add up in quadrature to about 2^-24 S: the worst-case K 2^-24 S, and the sqrt(K) 2^-24 S that holds for any signs,
could not tell the fp32 path from a bf16-rounded one at K = 1024; every epilogue operand and the stored value cost one more
rounding each; ELU' <= 1 and the factor of MUL_DELU <= 1 pass no more than the accumulator's error).  colsum: CONST * 2^-24 * sum_k |b_kn|.
The constants come from a float32 restatement on the CPU (restate32: 16-wide K chunks dealt over four partial sums, not torch's order)
which has to stay within RESTATEMENT_SHARE of every bound -- never from a GPU result.  Precision 1 uses the same bound: the products of
bf16 operands are exact in float32, so only the summation is left, and whether the bf16 MFMA's internal summation stays inside is what
the GPU test measures."""
import functools

import torch

from fold_cases import BF16, F32, SENTINEL, _elu_output, _rounded, assert_bits, elu_prime  # noqa: F401

NAN = float("nan")
U32 = 2.0 ** -24
RESTATEMENT_SHARE = 0.25            # the project's figure: the float32 restatement of every comparison stays within this share of its bound
DEFECT_MARGIN = 4.0                 # every planted defect exceeds the bound by at least this factor (host test)
# one constant per group letter: R single entries (air_gemm / air_gemm_bf16 / air_linear_*), S the tile families of air_gemm_grouped,
# T the wide-tile kernels, U the big-group kernels.  Set from restate32: with a constant of 1 its worst shares of the bound are 2.38 (R: the
# worst of two million elements at K = 20), 2.51 (S, K = 64), 1.96 (T, K = 256) and 2.71 (U: a colsum over K = 256), so these constants
# bring every group under RESTATEMENT_SHARE (tests/test_gemm_cases_host.py prints the shares they leave).
CONST = {"R": 12.0, "S": 12.0, "T": 10.0, "U": 12.0}
EPI_NONE, EPI_BIAS, EPI_BIAS_ELU, EPI_MUL_DELU, EPI_ADD_AUX, EPI_ADD_AUX_ELU = range(6)
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
LNAME = {(0, 0): "nn", (0, 1): "nt", (1, 0): "tn", (1, 1): "tt"}


def P(ta, tb, M, N, K, epi=EPI_NONE, beta=0.0, colsum=False, bias=None, pads=(0, 0, 0, 0), a_un=0, b_un=0, a16=False, b16=False,
      c16=False, apro=None, share_b=None):
    """one problem: pads = extra columns of (A, B, C, aux) rows; a_un / b_un: the operand starts that many floats past a 16-byte
    boundary; a16 / b16 / c16: bf16 mirrors given; apro: None | "lin" | "elu" (the A prologue a = act(A + A2 + a_bias), with a_out); share_b: B is the A operand of that earlier
    problem of the row (the same buffer: dy of air_linear_bwd)"""
    if bias is None:
        bias = epi in (EPI_BIAS, EPI_BIAS_ELU)
    return dict(ta=ta, tb=tb, M=M, N=N, K=K, epi=epi, beta=float(beta), colsum=bool(colsum), bias=bool(bias), pads=tuple(pads),
                a_un=a_un, b_un=b_un, a16=a16, b16=b16, c16=c16, apro=apro, share_b=share_b)


CASES = {}


def _case(name, entry, precision, problems, form, group, ws=None):
    """entry: "gemm" (air_gemm / air_gemm_bf16 by precision), "linear_fwd", "linear_bwd", "grouped"; ws: bytes of workspace offered
    ("gemm" only; None = the whole workspace, 0 = none); form: the fields of AirGemmForm the row expects (family by name)"""
    assert name not in CASES, name
    CASES[name] = dict(name=name, entry=entry, precision=precision, problems=problems, form=form, group=group, ws=ws)


def _tile(mt, kw, grouped, **kw_):
    return dict(family="tile", MT=mt, NT=mt, KW=kw, grouped=grouped, **kw_)


def _epi_kw(epi, i):
    """beta on every other epilogue, padded C / aux rows on the others"""
    return dict(epi=epi, beta=(0.5 if (epi + i) % 2 else 0.0), bias=(True if epi in (1, 2) else bool((epi + i) % 2 == 0 and epi >= 4)))


for prec in (F32, BF16):
    pn = "bf16" if prec else "f32"
    # ---- R. air_gemm / air_gemm_bf16 <1,1,4>, S = 1: every layout x every epilogue, beta, colsum with ta
    for li, (ta, tb) in enumerate(LAYOUTS):
        _case(f"gemm_{pn}_{LNAME[ta, tb]}_10x5x9", "gemm", prec, [P(ta, tb, 10, 5, 9, epi=li, beta=0.5 * (li == 3), colsum=ta, pads=(1, 2, 3, 0),
                                                                     a_un=li % 2)], _tile(1, 4, 0, S=1), "R")
        for epi in range(6):
            _case(f"gemm_{pn}_{LNAME[ta, tb]}_epi{epi}", "gemm", prec,
                  [P(ta, tb, 33, 47, 129, colsum=ta, pads=(li, 0, epi, 5 - epi), a_un=(epi + li) % 2, b_un=epi % 2, **_epi_kw(epi, li))],
                  _tile(1, 4, 0, S=1), "R")
    # ---- R. <1,1,4> with the cross-workgroup K split: K = 1030 = 64 chunks + a tail of 6; every epilogue, beta, ldc > N, ldaux > N;
    # the whole workspace (S = 4) and one that caps S at 2
    for epi in range(6):
        ta, tb = LAYOUTS[epi % 4]
        pr = P(ta, tb, 20, 24, 1030, pads=(0, 0, 4 + epi, 3), **_epi_kw(epi, 1))
        _case(f"gemm_{pn}_splitk4_epi{epi}", "gemm", prec, [pr], _tile(1, 4, 0, S=4, chunks_per_split=17), "R")
        _case(f"gemm_{pn}_splitk2_epi{epi}", "gemm", prec, [pr], _tile(1, 4, 0, S=2, chunks_per_split=33), "R", ws=2 * 20 * 24 * 4)
    # ---- R. <2,2,1>: 2080 tiles of 32 x 32, the four waves on four neighbouring N tiles; four layouts, every epilogue, beta, colsum
    for li, (ta, tb) in enumerate(LAYOUTS):
        for epi in ((li, li + 4) if li < 2 else (li,)):
            _case(f"gemm_{pn}_kw1_{LNAME[ta, tb]}_epi{epi}", "gemm", prec,
                  [P(ta, tb, 1010, 2050, 20, colsum=ta, pads=(li, 0, 2 * (epi % 2), 1), a_un=li % 2, **_epi_kw(epi, li))],
                  _tile(2, 1, 0, S=1, workgroups=32 * 17), "R")
    _case(f"gemm_{pn}_kw1_even", "gemm", prec, [P(1, 0, 1024, 2048, 20, colsum=True, beta=0.5)], _tile(2, 1, 0, S=1, workgroups=512), "R")
# the plain linear layer through the same body (fp32 only: air_linear_* call air_gemm)
_case("linear_fwd_kw1", "linear_fwd", F32, [P(0, 0, 1010, 2050, 20, epi=EPI_BIAS_ELU)], _tile(2, 1, 0, S=1), "R")
# air_linear_bwd(x[M, K], w[K, N], dy[M, N]) without activation launches dx[M, K] = dy . w^T and dw[K, N] = x^T . dy with db = colsum(dy): the
# row holds those two products as air_gemm sees them.  M = 37, K = 65540, N = 33 puts BOTH on <2,2,1> (2 x 2049 and 2049 x 2 tiles of 32 x 32,
# ragged in both dimensions) with contractions of 33 and 37: a 16-chunk tail each
LIN_M, LIN_K, LIN_N = 37, 65540, 33
_case("linear_bwd_kw1", "linear_bwd", F32, [P(0, 1, LIN_M, LIN_K, LIN_N), P(1, 0, LIN_K, LIN_N, LIN_M, colsum=True, share_b=0)],
      [_tile(2, 1, 0, S=1, workgroups=2 * 513), _tile(2, 1, 0, S=1, workgroups=2049)], "R")

# ---- S. air_gemm_grouped, the tile families.  The shapes of test_gemm_grouped_every_slot, and the lone-problem kernels of each
GROUP_SHAPES = {
    "tile16": [(16 + 4 * i, 8 + 5 * i, 64) + LAYOUTS[i % 4] for i in range(8)],
    "long_k": [(16, 4 + 4 * i, 512) + LAYOUTS[i % 4] for i in range(8)],
    "tile32": [(230, 200 + 9 * i, 16) + LAYOUTS[i % 4] for i in range(8)],
}
LONE_SHAPES = {"tile16": (37, 50, 70), "long_k": (20, 48, 520), "tile32": (810, 500, 24)}
TILE_FORM = {"tile16": (1, 4), "long_k": (1, 16), "tile32": (2, 4)}
for prec in (F32, BF16):
    pn = "bf16" if prec else "f32"
    for fam, shapes in GROUP_SHAPES.items():
        mt, kw = TILE_FORM[fam]
        probs = [P(ta, tb, M, N, K, colsum=bool(ta), pads=(i % 3, 0, i % 2, i % 4), a_un=i % 2, **_epi_kw(i % 6, i))
                 for i, (M, N, K, ta, tb) in enumerate(shapes)]
        _case(f"grouped_{pn}_{fam}", "grouped", prec, probs, _tile(mt, kw, 1, bf=prec), "S")
        M, N, K = LONE_SHAPES[fam]
        for li, (ta, tb) in enumerate(LAYOUTS[:3] if fam != "tile16" else LAYOUTS):
            _case(f"grouped_{pn}_{fam}_lone_{LNAME[ta, tb]}", "grouped", prec,
                  [P(ta, tb, M, N, K, colsum=bool(ta), pads=(li, 1, 2, 3), a_un=li % 2, **_epi_kw((li + 2) % 6, li))],
                  _tile(mt, kw, 0, bf=prec), "S")
    # the A prologue (lone problem, K % 16 == 0, everything 16-byte aligned), a_out in a sentinel parent
    _case(f"grouped_{pn}_apro", "grouped", prec, [P(0, 1, 37, 50, 64, epi=EPI_BIAS, pads=(4, 0, 3, 0), apro="lin")],
          dict(family="apro", MT=1, NT=1, KW=4, grouped=0, bf=prec), "S")
_case("grouped_f32_apro_elu", "grouped", F32, [P(0, 0, 21, 40, 32, pads=(0, 2, 0, 0), apro="elu")],
      dict(family="apro", MT=1, NT=1, KW=4, grouped=0, bf=0), "S")
# the c16 forms (bf16, the bf16 mirror of C written by the epilogue), single and grouped
for fam, shapes in GROUP_SHAPES.items():
    mt, kw = TILE_FORM[fam]
    probs = [P(ta, tb, M, N, K, colsum=bool(ta), pads=(0, 0, 2 * (i % 2), 0), c16=True, **_epi_kw(i % 6, i)) for i, (M, N, K, ta, tb) in enumerate(shapes)]
    _case(f"grouped_c16_{fam}", "grouped", BF16, probs, dict(family="c16", MT=mt, NT=mt, KW=kw, grouped=1, bf=1), "S")
    M, N, K = LONE_SHAPES[fam]
    _case(f"grouped_c16_{fam}_lone", "grouped", BF16, [P(0, 1, M, N, K, epi=EPI_BIAS_ELU, pads=(0, 0, 2, 0), c16=True)],
          dict(family="c16", MT=mt, NT=mt, KW=kw, grouped=0, bf=1), "S")
# the streaming short-K body: mixed with tile problems (16 x 16), all short-K, and beside more than 1536 tiles (32 x 32)
_sk = [P(ta, tb, M, N, K, pads=(i % 3, 0, i % 2, 0)) for i, (M, N, K, ta, tb) in enumerate(GROUP_SHAPES["tile16"])]
_sk[5] = P(1, 0, 4096, 64, 32, colsum=True)
_case("grouped_shortk_mixed", "grouped", F32, _sk, dict(family="shortk", MT=1, NT=1, KW=4, grouped=1, sk_mask=1 << 5, tile=16), "S")
_case("grouped_shortk_all", "grouped", F32, [P(1, 0, 4099, 64, 16, colsum=True), P(1, 0, 6163, 192, 48, colsum=True, pads=(1, 0, 0, 0))],
      dict(family="shortk", MT=1, NT=1, KW=4, grouped=1, sk_mask=3), "S")
_case("grouped_shortk_tile32", "grouped", F32, [P(1, 0, 4100, 128, 64), P(0, 0, 810, 500, 24, epi=EPI_BIAS)],
      dict(family="shortk", MT=2, NT=2, KW=4, grouped=1, sk_mask=1, tile=32), "S")

# ---- T. the wide-tile kernels: groups of just over 1000 16 x 16 tiles.  (layout, MT): TN 4, NN 1, NT with K >= 512 1, NT-short 2
WIDE = {  # name: (ta, tb, [(M, N, K)], lone (M, N, K))
    "tn": (1, 0, [(128, 208 + 16 * i, 256) for i in range(8)], (520, 516, 256)),
    "nn": (0, 0, [(128, 208 + 16 * i, 20) for i in range(8)], (126, 2064, 20)),
    "nt": (0, 1, [(125, 1040, 512), (128, 1100, 516)], (125, 2063, 512)),
}
for name, (ta, tb, shapes, lone) in WIDE.items():
    mt = 4 if ta else 1
    wf = dict(family="wide", MT=mt, KW=8, ta=ta, tb=tb, bf=0)
    probs = [P(ta, tb, M, N, K, colsum=bool(ta), pads=(4 * (i % 2), 4, i % 3, i % 2), **_epi_kw(i % 6, i)) for i, (M, N, K) in enumerate(shapes)]
    _case(f"wide_f32_{name}", "grouped", F32, probs, dict(wf, grouped=1), "T")
    _case(f"wide_f32_{name}_lone", "grouped", F32, [P(ta, tb, *lone, colsum=bool(ta), pads=(4, 0, 3, 0), epi=EPI_BIAS, beta=0.5)], dict(wf, grouped=0), "T")
# K = 1024: the XCD-contiguous tile map; 1105 tiles of 16 x 16 / 85 workgroups, not a multiple of 8
_case("wide_f32_tn_xcd", "grouped", F32, [P(1, 0, 260, 516, 1024, colsum=True), P(1, 0, 264, 512, 1028)],
      dict(family="wide", MT=4, KW=8, ta=1, tb=0, grouped=1, xcd_map=1, workgroups=5 * 9 + 5 * 8), "T")
# above 2048 tiles: an unaligned A, K % 4 != 0 for NN, K < 16
_case("wide_f32_nn_far", "grouped", F32, [P(0, 0, 253, 2064, 10, epi=EPI_BIAS, pads=(1, 0, 1, 0), a_un=1), P(0, 0, 64, 132, 7, pads=(2, 4, 0, 0))],
      dict(family="wide", MT=1, KW=8, ta=0, tb=0, grouped=1), "T")
# wide16, the bf16 data path: NN, NT (K >= 512) and NT-short (above 2048 tiles) with all four mirror combinations, C16 written.
# (bf16 TN groups go to the big-group launch: U.)
WIDE16 = {
    "nn": (0, 0, 1, [(128, 1032, 20), (125, 1036, 24)], (126, 2064, 20)),
    "nt": (0, 1, 1, [(125, 1040, 512), (128, 1100, 516)], (125, 2063, 512)),
    "nts": (0, 1, 2, [(253, 1040, 20), (250, 1100, 24)], (250, 2130, 12)),
}
for name, (ta, tb, mt, shapes, lone) in WIDE16.items():
    for a16 in (0, 1):
        for b16 in (0, 1):
            wf = dict(family="wide16", MT=mt, KW=8, ta=ta, tb=tb, bf=1, nt_short=int(mt == 2))
            probs = [P(ta, tb, M, N, K, pads=(4 * (i % 2), 4, i % 3, i % 2), a16=a16, b16=b16, c16=True, **_epi_kw((i + a16 + 2 * b16) % 6, i))
                     for i, (M, N, K) in enumerate(shapes)]
            _case(f"wide16_{name}_a{a16}b{b16}", "grouped", BF16, probs,
                  dict(wf, grouped=1, a16_mask=3 * a16, b16_mask=3 * b16), "T")
            _case(f"wide16_{name}_a{a16}b{b16}_lone", "grouped", BF16,
                  [P(ta, tb, *lone, pads=(4, 0, 3, 0), epi=EPI_BIAS_ELU, a16=a16, b16=b16, c16=bool(a16 ^ b16))],
                  dict(wf, grouped=0, a16_mask=a16, b16_mask=b16), "T")

# ---- U. the big group: more than 8 and up to 24 TN problems, small_mask members (M = 1..3, N = 1), per-problem mirror kinds
_big = [P(1, 0, 64 + 4 * (i % 5), 68 + 4 * (i % 3), 40 + 4 * i, colsum=bool(i % 2), pads=(i % 2, 4 * (i % 2), i % 3, 0)) for i in range(9)]
_big += [P(1, 0, 1 + i % 3, 1, 45 + i, colsum=True) for i in range(3)] + [P(1, 0, 50, 6, 33, pads=(1, 0, 0, 0)), P(0, 0, 20, 24, 9, epi=EPI_BIAS)]
_case("big_f32_14", "grouped", F32, _big, dict(family="big", MT=4, KW=8, grouped=1, small_mask=0b11111 << 9, xcd_map=0), "U")
_case("big_bf16_14", "grouped", BF16,
      [dict(p, a16=bool(i % 2), b16=bool(i % 3 == 0), pads=(2 * (i % 2), p["pads"][1], p["pads"][2], 0)) for i, p in enumerate(_big)],
      dict(family="big16", MT=4, KW=8, grouped=1, small_mask=0b11111 << 9, xcd_map=0, a16_mask=0b0010101010, b16_mask=(1 << 0 | 1 << 3 | 1 << 6 | 1 << 12)), "U")
_big24 = [P(1, 0, 68, 72, 1024 + 4 * i) for i in range(21)] + [P(1, 0, 2, 1, 1030, colsum=True), P(1, 0, 3, 1, 77), P(1, 0, 1, 1, 5)]
_case("big_f32_24_xcd", "grouped", F32, _big24, dict(family="big", grouped=1, small_mask=0b111 << 21, xcd_map=1, workgroups=21 * 4 + 3), "U")
_case("big_bf16_24_xcd", "grouped", BF16, [dict(p, a16=bool(i % 2), b16=bool(i % 2)) for i, p in enumerate(_big24)],
      dict(family="big16", grouped=1, small_mask=0b111 << 21, xcd_map=2, workgroups=21 * 4 + 3), "U")
# up to 8 bf16 TN problems in the wide regime: handed over to the big-group launch
_case("big_bf16_handover", "grouped", BF16, [P(1, 0, M, N, K, colsum=True, a16=bool(i % 2), b16=True) for i, (M, N, K) in enumerate(WIDE["tn"][2])],
      dict(family="big16", grouped=1, small_mask=0, xcd_map=0, a16_mask=0b10101010, b16_mask=255), "U")
# K = 768 = 24 chunks of 32 with both mirrors: two chunks in flight per wave, the second group short.  The colsum of this form counted
# the re-read last chunks twice until this suite found it (gemm_wide16_body, csrc/gemm_kernels.hip).
_case("big_bf16_9_k768", "grouped", BF16, [P(1, 0, 64, 68 + 4 * (i % 2), 768 + 32 * (i % 3), colsum=True, a16=True, b16=True) for i in range(9)],
      dict(family="big16", grouped=1, small_mask=0, a16_mask=511, b16_mask=511, xcd_map=0), "U")
_case("big_bf16_handover_lone", "grouped", BF16, [P(1, 0, 520, 516, 256, colsum=True)],
      dict(family="big16", grouped=1, small_mask=0, a16_mask=0, b16_mask=0), "U")


# ---------------------------------------------------------------------------------------------------------------
# the reachable set: every (entry, family, template arguments, precision) the launch switches of gemm_dispatch and air_gemm_grouped
# can reach.  Written from the switch, not from the table.
# ---------------------------------------------------------------------------------------------------------------
def form_key(entry, precision, form):
    """what identifies a kernel instantiation: family, grouped or lone kernel, template arguments, precision (and S > 1 for the
    split-K epilogue kernel of air_gemm)"""
    fam = form["family"]
    key = [entry, fam, form["grouped"], form["MT"], form["KW"], precision]
    if fam in ("wide", "wide16"):
        key += [form["ta"], form["tb"]]
    if fam == "wide16":
        key += [int(form["a16_mask"] != 0), int(form["b16_mask"] != 0)]
    if entry != "grouped":
        key += [int(form["S"] > 1)]
    return tuple(key)


def reachable():
    keys = set()
    for prec in (F32, BF16):
        keys |= {("gemm", "tile", 0, 1, 4, prec, 0), ("gemm", "tile", 0, 1, 4, prec, 1), ("gemm", "tile", 0, 2, 1, prec, 0)}   # gemm_dispatch
        for grouped in (0, 1):
            for mt, kw in ((1, 16), (1, 4), (2, 4)):
                keys.add(("grouped", "tile", grouped, mt, kw, prec))                 # AIR_SINGLE_LAUNCH / AIR_GROUP_LAUNCH
                if prec == BF16:
                    keys.add(("grouped", "c16", grouped, mt, kw, prec))              # AIR_C16_LAUNCH
        keys.add(("grouped", "apro", 0, 1, 4, prec))
    # air_linear_fwd / air_linear_bwd call air_gemm: held where the plain entries' tests never were, on <2,2,1>
    keys |= {("linear_fwd", "tile", 0, 2, 1, F32, 0), ("linear_bwd", "tile", 0, 2, 1, F32, 0)}
    keys |= {("grouped", "shortk", 1, 1, 4, F32), ("grouped", "shortk", 1, 2, 4, F32)}  # gemm_grouped_sk_kernel<1,1> / <2,2>
    for grouped in (0, 1):
        # AIR_WIDE_LAUNCH: <4, TN>, <1, NT>, <1, NN>.  <2, NT> (NT-short) is in the switch but wide_group_eligible admits it with
        # bf16 operands only, and <4, TN> of AIR_WIDE16_LAUNCH never runs from here: a bf16 TN group goes to the big-group launch
        keys |= {("grouped", "wide", grouped, 4, 8, F32, 1, 0), ("grouped", "wide", grouped, 1, 8, F32, 0, 1), ("grouped", "wide", grouped, 1, 8, F32, 0, 0)}
        for mt, ta, tb in ((2, 0, 1), (1, 0, 1), (1, 0, 0)):
            for a16 in (0, 1):
                for b16 in (0, 1):
                    keys.add(("grouped", "wide16", grouped, mt, 8, BF16, ta, tb, a16, b16))
    keys |= {("grouped", "big", 1, 4, 8, F32), ("grouped", "big16", 1, 4, 8, BF16)}
    return keys


# ---------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------
class View:
    """a [rows, cols] window with leading dimension ld, `lead` elements into a flat parent (CPU; .on(parent) re-forms the window on a
    copy of the parent, e.g. on the device)"""

    def __init__(self, rows, cols, ld, lead, fill, dtype=torch.float32, tail=None):
        self.rows, self.cols, self.ld, self.lead = rows, cols, ld, lead
        tail = max(2 * ld, 8) if tail is None else tail
        self.parent = torch.full((lead + rows * ld + tail,), fill, dtype=dtype)

    def on(self, parent):
        return parent[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    @property
    def v(self):
        return self.on(self.parent)

    def outside(self, parent):
        """the elements of `parent` (a copy on any device) outside the window, as one flat tensor"""
        mask = torch.ones(self.parent.numel(), dtype=torch.bool)
        self.on(mask).fill_(False)
        return parent.detach().cpu()[mask]

    def byte_offset(self):
        return self.lead * self.parent.element_size()


def _lead(ld, un):
    return (2 * ld + 3) // 4 * 4 + un


def _signed(gen, rows, cols, quantum=None):
    x = (0.5 + torch.rand(rows, cols, generator=gen)) * (torch.randint(0, 2, (rows, cols), generator=gen) * 2 - 1).float()
    if quantum:
        x = torch.round(x / quantum) * quantum
    return x


def _operand(gen, rows, cols, pad, un, quantum=None):
    v = View(rows, cols, cols + pad, _lead(cols + pad, un), NAN)
    v.v.copy_(_signed(gen, rows, cols, quantum))
    return v


def _mirror(src):
    """the bf16 mirror of an operand: the same window of a NaN-filled bf16 parent"""
    m = View(src.rows, src.cols, src.ld, src.lead, NAN, dtype=torch.bfloat16)
    m.v.copy_(src.v.to(torch.bfloat16))
    return m


def elu64(x):
    return torch.where(x > 0, x, torch.expm1(x))


def epilogue(acc, pr, d, kind=torch.float64):
    """apply_epilogue (csrc/gemm_kernels.hip) in `kind` on the accumulator: acc + beta C0, then the epilogue"""
    c = lambda k: d[k].v.to(kind)
    v = acc
    if pr["beta"] != 0.0:
        v = v + torch.tensor(pr["beta"], dtype=kind) * c("C0")
    e = pr["epi"]
    if e in (EPI_BIAS, EPI_BIAS_ELU):
        v = v + c("bias")[0]
    elif e == EPI_MUL_DELU:
        v = v * elu_prime(c("aux"))
    elif e in (EPI_ADD_AUX, EPI_ADD_AUX_ELU):
        v = v + c("aux")
        if pr["bias"]:
            v = v + c("bias")[0]
    return elu64(v) if e in (EPI_BIAS_ELU, EPI_ADD_AUX_ELU) else v


def op_a32(pr, d):
    """the float32 A operand the product sees, [M, K]: with the prologue, act(A + A2 + a_bias) -- exact in float32 for "lin" (all three
    are multiples of 2^-6 of small magnitude)"""
    a = d["A"].v
    if pr["apro"]:
        a = a + d["A2"].v + d["a_bias"].v[0]
        if pr["apro"] == "elu":
            a = elu64(a.double()).float()
    return a.t() if pr["ta"] else a


@functools.lru_cache(maxsize=4)
def data(name):
    """the case's problems as dicts of Views (inputs filled, C0 only where beta != 0) and float64 references: out64, S, bound, colsum64,
    colsum_bound, a64 (the prologue's a_out)"""
    case = CASES[name]
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31))
    r = _rounded(case["precision"])
    out = []
    for pr in case["problems"]:
        M, N, K, ta, tb = pr["M"], pr["N"], pr["K"], pr["ta"], pr["tb"]
        pa, pb, pc, paux = pr["pads"]
        q = 2.0 ** -6 if pr["apro"] else None
        d = dict(A=_operand(gen, K if ta else M, M if ta else K, pa, pr["a_un"], q))
        d["B"] = out[pr["share_b"]]["A"] if pr["share_b"] is not None else _operand(gen, N if tb else K, K if tb else N, pb, pr["b_un"])
        assert (d["B"].rows, d["B"].cols) == ((N, K) if tb else (K, N))
        if pr["apro"]:
            d["A2"] = View(M, K, K + pa, _lead(K + pa, 0), NAN)
            d["A2"].v.copy_(torch.round((torch.rand(M, K, generator=gen) - 0.5) * 16) / 64)            # |A2| <= 1/8
            d["a_bias"] = View(1, K, K, 8, NAN)
            d["a_bias"].v.copy_(torch.round((torch.rand(1, K, generator=gen) - 0.5) * 16) / 64)
        if pr["bias"]:
            d["bias"] = View(1, N, N, 5, NAN)
            d["bias"].v.copy_(_signed(gen, 1, N))
        if pr["epi"] >= EPI_MUL_DELU:
            d["aux"] = View(M, N, N + paux, _lead(N + paux, 1), NAN)
            d["aux"].v.copy_(_elu_output(gen, M, N) if pr["epi"] == EPI_MUL_DELU else _signed(gen, M, N))
        if pr["beta"] != 0.0:
            d["C0"] = View(M, N, N + pc, _lead(N + pc, 0), SENTINEL)
            d["C0"].v.copy_(_signed(gen, M, N))
        a32, b32 = op_a32(pr, d), (d["B"].v.t() if tb else d["B"].v)
        a64, b64 = r(a32).double(), r(b32).double()
        acc = a64 @ b64
        S = a64.abs() @ b64.abs()
        d["acc64"], d["S"] = acc, S
        d["out64"] = epilogue(acc, pr, d)
        mag = S + d["out64"].abs()
        for k, scale in (("C0", abs(pr["beta"])), ("bias", 1.0), ("aux", 1.0)):
            if k in d and not (k == "aux" and pr["epi"] == EPI_MUL_DELU):
                mag = mag + scale * d[k].v.double().abs()
        if pr["epi"] in (EPI_BIAS_ELU, EPI_ADD_AUX_ELU):
            mag = mag + 1.0
        if pr["apro"] == "elu":
            mag = mag + 8.0 * S                    # a = elu(.) is formed in float32: a few units in every operand of every term
        d["mag"] = mag
        if pr["colsum"]:
            d["colsum64"] = b32.double().sum(0)
            d["colsum_mag"] = b32.double().abs().sum(0)
        if pr["apro"]:
            d["a32"] = a32
        assert bool(torch.isfinite(d["out64"]).all())
        out.append(d)
    return out


def bound(case, d):
    return CONST[case["group"]] * U32 * d["mag"]


def colsum_bound(case, d):
    return CONST[case["group"]] * U32 * d["colsum_mag"]


# ---------------------------------------------------------------------------------------------------------------
# the float32 restatement: the product over 16-wide K chunks dealt round-robin to four partial sums (each a plain multiply-then-add
# loop in float32), the partial sums added in order, the epilogue in float32 -- not torch's summation order, and no fma
# ---------------------------------------------------------------------------------------------------------------
def product32(a, b):
    """a[M, K], b[K, N] float32 -> float32 [M, N]"""
    M, K = a.shape
    parts = [torch.zeros(M, b.shape[1]) for _ in range(4)]
    for k in range(K):
        w = (k // 16) % 4
        parts[w] = parts[w] + a[:, k:k + 1] * b[k:k + 1, :]
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def restate32(case, pr, d):
    """-> out32, colsum32 | None"""
    r = _rounded(case["precision"])
    a32, b32 = op_a32(pr, d), (d["B"].v.t() if pr["tb"] else d["B"].v)
    acc = product32(r(a32).float().contiguous(), r(b32).float().contiguous())
    out = epilogue(acc, pr, d, torch.float32)
    cs = None
    if pr["colsum"]:
        cs = torch.zeros(b32.shape[1])
        for k in range(b32.shape[0] - 1, -1, -1):
            cs = cs + b32[k]
    return out, cs


# ---------------------------------------------------------------------------------------------------------------
# descriptors for the host mirror and the library's query: pointers as integers.  Every parent sits at a base aligned to 256 bytes.
# ---------------------------------------------------------------------------------------------------------------
def descs(name, base=1 << 24):
    from attend_infer_repeat_amd import _lib
    case, out = CASES[name], []
    nxt = [base]

    def addr(view_lead_bytes):
        a = nxt[0] + view_lead_bytes
        nxt[0] += 1 << 24
        return a

    for pr, d in zip(case["problems"], data(name)):
        M, N, K = pr["M"], pr["N"], pr["K"]
        A, B = d["A"], d["B"]
        ldc = N + pr["pads"][2]
        dd = _lib.AirGemmDesc(pr["ta"], pr["tb"], M, N, K, addr(A.byte_offset()), A.ld, addr(B.byte_offset()), B.ld, addr(4 * _lead(ldc, 0)), ldc,
                              addr(20) if pr["bias"] else None, pr["epi"], addr(d["aux"].byte_offset()) if "aux" in d else None,
                              d["aux"].ld if "aux" in d else 0, pr["beta"], addr(16) if pr["colsum"] else None, case["precision"],
                              addr(d["A2"].byte_offset()) if pr["apro"] else None, addr(32) if pr["apro"] else None,
                              int(pr["apro"] == "elu"), addr(4 * A.lead) if pr["apro"] else None)
        if pr["a16"]:
            dd.A16 = addr(2 * A.lead)
        if pr["b16"]:
            dd.B16 = addr(2 * B.lead)
        if pr["c16"]:
            dd.C16 = addr(2 * _lead(ldc, 0))
        out.append(dd)
    return out
