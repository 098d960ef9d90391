"""GEMM grouping policy of the train-step plans: which problems share a launch.  Pure arithmetic over `AirGemmDesc` fields -- no
torch, no device, no library handle -- so it runs (and is tested) on the host.  Every function takes descriptors and returns lists
of groups of descriptors; the caller (engine_plan.py) turns each group into an array, keeps it alive and appends the plan entry.

Three policies live here:
  plan_launch          the rule of every grouped launch of the forward and the backward;
  deferred_dw_groups   the weight gradients the throughput regime forms at the end of the backward;
  wide_form / shortk_mixed / tensors_read / foldable   what the folded closing update (engine_plan._fold_closing_update) must know
                       of the library's dispatch and of the flat buffers before it folds an update into a grouped launch;
  latency_tile / group_long_k / on_long_k_body / shortk_eligible / shortk_workgroups / latency_form / gather_fits / first_step_fits /
  lstm_fwd_wide / lstm_bwd_form / lstm_bwd_entry_fits / lstm_bf16_fits        the tile-form rules of the latency-regime grouped launches and of the LSTM step
                       (tests/test_fold_cases_host.py holds every kernel-level case against them);
  grouped_form / single_form   the WHOLE dispatch rule of air_gemm_grouped and of air_gemm / air_gemm_bf16 -- kernel family, template
                       arguments and what follows from them -- field for field what the library's own queries air_gemm_grouped_form /
                       air_gemm_form return (tests/test_gemm_cases_host.py holds the two against each other).
The predicates restate rules of the library (csrc/gemm_kernels.hip, csrc/lstm_kernels.hip); each names the function it mirrors."""
from . import _lib

GROUPED, SPLITK = "grouped", "splitk"      # kinds of plan_launch: air_gemm_grouped / the split-K single-GEMM entry (air_gemm, air_gemm_bf16)


def tiles16(d):
    return ((d.M + 15) // 16) * ((d.N + 15) // 16)


def is_weight_gradient(d):
    """a TN problem: K = rows of the batch, a small output nothing but the optimiser consumes"""
    return bool(d.ta and not d.tb)


def wide_ok(d, group_tiles16):
    """what air_gemm_grouped's wide-tile kernels need of a problem (gemm_kernels.hip wide_group_eligible)"""
    strict = group_tiles16 > 2048 or (d.A % 16 == 0 and d.lda % 4 == 0 and d.K % 4 == 0)
    return bool(strict and not (d.ta and d.tb) and not d.A2 and d.B % 16 == 0 and d.ldb % 4 == 0
                and (not (d.ta or d.tb) or d.K % 4 == 0) and d.M >= 4 and d.N >= 4 and d.K >= 4
                and (not d.ta or d.M % 4 == 0) and (d.tb or d.N % 4 == 0))


def plan_launch(descs, throughput, use16, allow_splitk=False):
    """[(kind, problems)]: the launches that dispatch `descs`, in order.  kind SPLITK: a lone long-K problem for the split-K
    single-GEMM entry; GROUPED: up to 8 problems for air_gemm_grouped."""
    total = sum(tiles16(d) for d in descs)
    if throughput and len(descs) > 1:
        ok = [wide_ok(d, total) for d in descs]
        if any(ok) and not all(ok):
            # one odd problem (N = 1, K = 50 ...) would keep the whole group off the wide-tile kernels: it gets its own launch
            return (plan_launch([d for d, w in zip(descs, ok) if w], throughput, use16)
                    + plan_launch([d for d, w in zip(descs, ok) if not w], throughput, use16))
    if (len(descs) == 1 and allow_splitk and descs[0].K >= 1024 and total > 256 and not use16
            and not (throughput and wide_ok(descs[0], total))):
        return [(SPLITK, list(descs))]
    groups = [descs]
    if total > 1536 and len(descs) > 1:
        # large batch: launches are cheap relative to the work, and the library picks ONE tile shape / K-split per
        # launch -- keep the long-K few-tile problems (weight gradients: K = T*B) apart from the many-tile ones
        is_long = lambda d: d.K >= 1024 and tiles16(d) <= 1024
        groups = [g for g in ([d for d in descs if is_long(d)], [d for d in descs if not is_long(d)]) if g]
    return [(GROUPED, list(grp[i:i + 8])) for grp in groups for i in range(0, len(grp), 8)]


# ---- deferred weight gradients (throughput regime) ------------------------------------------------------------------------------
def deferred_wide_ok(d):
    """16-byte loads along M and N: both multiples of 4, aligned"""
    return bool(d.M % 4 == 0 and d.M >= 4 and d.N % 4 == 0 and d.ldb % 4 == 0 and d.K % 4 == 0 and d.B % 16 == 0)


def split_rows(d):
    """a row count that is not a multiple of 4 (50 latent / 677 baseline-input rows): the first M - M % 4 rows go wide, the
    remaining one to three rows are a problem of their own (the bias gradient stays with the first part)"""
    m4 = d.M // 4 * 4
    if not (d.M % 4 and m4 >= 16 and d.N % 4 == 0 and d.ldb % 4 == 0 and d.K % 4 == 0 and d.B % 16 == 0):
        return [d]
    return [_lib.AirGemmDesc(d.ta, d.tb, m4, d.N, d.K, d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.bias,
                             d.epilogue, d.aux, d.ldaux, d.beta, d.colsum, d.precision, None, None, 0, None),
            _lib.AirGemmDesc(d.ta, d.tb, d.M - m4, d.N, d.K, d.A + 4 * m4, d.lda, d.B, d.ldb,
                             d.C + 4 * m4 * d.ldc, d.ldc, d.bias, d.epilogue, d.aux, d.ldaux, d.beta, None,
                             d.precision, None, None, 0, None)]


def pack(problems, n_wide):
    """launches of up to 24 problems while wide-tile members are among them (the library's mixed form needs at
    least one), of up to 8 otherwise; the first `n_wide` of `problems` are the wide-tile eligible ones"""
    out, i = [], 0
    while i < len(problems):
        step = 24 if i < n_wide else 8
        chunk = problems[i:i + step]
        if len(chunk) <= 8 and i < n_wide < i + len(chunk):     # (8 or fewer go through the all-one-kind launches)
            out += [problems[i:n_wide], problems[n_wide:i + len(chunk)]]
        else:
            out.append(chunk)
        i += step
    return out


def deferred_dw_groups(deferred, bf16):
    """the launches of the deferred weight gradients: wide-tile eligible problems together, longest K first so that the heaviest
    tiles start first; the rest (M = 50 / 677 / 1, N = 1) behind them.  The library takes up to 24 problems in one launch when at
    least one is wide-tile eligible: the odd-shaped rest (one to three rows, a single column: eight long-K reductions) rides in
    the same grid on 16x16 tiles instead of costing a 14.5 us launch of its own."""
    parts = [q for d in deferred for q in split_rows(d)]
    wide = sorted((d for d in parts if deferred_wide_ok(d)), key=lambda d: (-d.K, -d.M * d.N))
    rest = [d for d in parts if not deferred_wide_ok(d)]
    if not bf16:
        # fp32 (MFMA-issue bound tiles): ONE launch for everything -- long-K tiles first, the CUs that finish early keep
        # pulling short-K tiles instead of idling until a launch of their own (batch 1024: 0.636 -> 0.607 ms)
        return pack(wide + rest, len(wide))
    # bf16 operands (L2 / L1 traffic bound tiles): the long-K problems in a launch of 8 with the grid-wide
    # XCD-contiguous tile map, the others + the rest in a second one (0.474 against 0.485 ms for a single launch)
    return ([wide[:8]] if wide[:8] else []) + pack(wide[8:] + rest, len(wide[8:]))


# ---- what the folded closing update asks of a grouped launch -----------------------------------------------------------------------
def wide_form(descs, wide_min_tiles):
    """the library declines (AIR_E_UNSUPPORTED) to fold an update into a group its wide-tile dispatch would take -- all weight
    gradients, K >= 256, more than AIR_GEMM_WIDE_MIN_TILES 16x16 tiles (a long batch at T = 1; gemm_kernels.hip
    wide_regime_weight_gradients): such a plan keeps its closing launch"""
    return (sum(tiles16(d) for d in descs) > wide_min_tiles and all(is_weight_gradient(d) for d in descs)
            and min(d.K for d in descs) >= 256)


def shortk_eligible(d, min_m):
    """gemm_kernels.hip shortk_eligible: what the streaming body takes -- an fp32 TN weight gradient with no epilogue, K in
    {16, 32, 48, 64}, N a multiple of 64 up to 256, at least AIR_GEMM_SHORTK_MIN_M (`min_m`) output rows"""
    return bool(is_weight_gradient(d) and d.precision == 0 and 16 <= d.K <= 64 and d.K % 16 == 0 and 64 <= d.N <= 256 and d.N % 64 == 0
                and d.M >= min_m and d.epilogue == 0 and d.beta == 0.0 and not d.bias and not d.A2 and not d.C16)


def shortk_workgroups(M, cap=384):
    """gemm_kernels.hip shortk_workgroups: one workgroup per 16-row slab up to AIR_GEMM_SHORTK_WGS (`cap`); beyond, the slabs go round"""
    return min((M + 15) // 16, max(cap, 1))


def shortk_mask(descs, enabled, min_m):
    """gemm_kernels.hip shortk_mask: the problems of a plain fp32 group that go to the streaming body (0: none, or not such a group)"""
    if not enabled or any(d.A2 or d.C16 or d.precision != 0 for d in descs):
        return 0
    return sum(1 << i for i, d in enumerate(descs) if shortk_eligible(d, min_m))


def shortk_mixed(descs, enabled, min_m):
    """... and a group that MIXES a short-K streaming weight gradient (shortk_eligible) with tile problems: such a problem keeps
    the product of the streaming body in every plan, and the folded launch takes it only when all its problems are of that kind"""
    mask = shortk_mask(descs, enabled, min_m)
    return mask != 0 and mask != (1 << len(descs)) - 1


def latency_tile(group_tiles16):
    """gemm_kernels.hip latency_tile: 16x16 tiles while the group is far from filling the chip, 32x32 beyond 1536 of them"""
    return 32 if group_tiles16 > 1536 else 16


def long_k(M, N, K):
    """air_common.h air_gemm_long_k: per problem, K >= 512 and >= 8 min(M, N)"""
    return K >= 512 and K >= 8 * min(M, N)


def group_long_k(descs):
    """gemm_kernels.hip group_long_k: the 16-wave K-split body -- at most 1024 tiles, every problem long_k"""
    return sum(tiles16(d) for d in descs) <= 1024 and all(long_k(d.M, d.N, d.K) for d in descs)


def on_long_k_body(descs, wide_min_tiles=1000):
    """gemm_kernels.hip group_on_long_k_body: a group air_gemm_grouped is sure to run on the 16-wave K-split body -- group_long_k, and
    too few tiles for the wide-tile regime, which air_gemm_grouped tests first"""
    return sum(tiles16(d) for d in descs) <= wide_min_tiles and group_long_k(descs)


def lone_on_tile16_kw4(M, N, K, wide_min_tiles=1000):
    """air_common.h air_gemm_lone_on_tile16_kw4: a lone problem air_gemm_grouped runs on the 4-wave 16x16 body whatever its layout and
    alignment -- too few tiles for the wide-tile regime and for 32x32 tiles, and not the long-K split"""
    t = ((M + 15) // 16) * ((N + 15) // 16)
    return t <= wide_min_tiles and latency_tile(t) == 16 and not long_k(M, N, K)


def first_step_fits(M, Hd, E, wide_min_tiles=1000, max_tiles=512):
    """lstm_kernels.hip air_lstm_first_step_fwd: at most 512 tiles of (batch, hidden), and a gx product [M, 4Hd, E] that as a launch of
    its own runs on the 4-wave 16x16 body, whose K order the first step repeats (bit-identical either way, or not folded)"""
    return ((M + 15) // 16) * ((Hd + 15) // 16) <= max_tiles and lone_on_tile16_kw4(M, 4 * Hd, E, wide_min_tiles)


FIRST_STEP_MAX_TILES = 512      # air_lstm_first_step_fwd, and the edge between lstm_fwd_fused_kernel and lstm_fwd_wide_kernel


def lstm_fwd_wide(M, Hd, ldw=None, ldh=None, w_h=0, h_prev=0):
    """lstm_kernels.hip lstm_fwd_launch: the 512-thread lstm_fwd_wide_kernel (else lstm_fwd_fused_kernel) -- more than 512 tiles of
    (batch, hidden), Hd a multiple of 64, rows of W_h [Hd, ldw = 4 Hd] and of h_prev [M, ldh = Hd; 0: one broadcast row] whole
    float4s, both at 16-byte aligned byte addresses `w_h` / `h_prev`"""
    ldw, ldh = 4 * Hd if ldw is None else ldw, Hd if ldh is None else ldh
    return bool(((M + 15) // 16) * ((Hd + 15) // 16) > FIRST_STEP_MAX_TILES and Hd % 64 == 0 and ldw % 4 == 0 and ldh % 4 == 0
                and w_h % 16 == 0 and h_prev % 16 == 0)


def lstm_bwd_form(M, Hd, dgates_next=0, w_h=0):
    """lstm_kernels.hip lstm_bwd_launch: the body of one BPTT link (air_lstm_step_bwd[_opt]) -- "kw16": lstm_bwd_fused_kernel<16> up to
    512 tiles of (batch, hidden); beyond, "wide": lstm_bwd_wide_kernel where Hd is a multiple of 64 and dgates_next [M, 4 Hd] and
    w_h [Hd, 4 Hd] lie at 16-byte aligned byte addresses `dgates_next` / `w_h` (vecA, vecB), else "kw4": lstm_bwd_fused_kernel<4>"""
    tiles = ((M + 15) // 16) * ((Hd + 15) // 16)
    if tiles > FIRST_STEP_MAX_TILES and Hd % 64 == 0 and dgates_next % 16 == 0 and w_h % 16 == 0:
        return "wide"
    return "kw16" if tiles <= FIRST_STEP_MAX_TILES else "kw4"


def lstm_bwd_entry_fits(M, Hd):
    """lstm_kernels.hip air_lstm_step_bwd_entry_fits: the entry of the BPTT folded into its first link (lstm_bwd_entry_kernel) -- whole
    16-unit chunks and at most 512 tiles of (batch, hidden)"""
    return bool(M > 0 and Hd > 0 and Hd % 16 == 0 and ((M + 15) // 16) * (Hd // 16) <= FIRST_STEP_MAX_TILES)


def lstm_bf16_fits(M, Hd):
    """lstm_kernels.hip air_lstm_step_fwd_bf16 / air_lstm_step_bwd_bf16: the shape rule of the steps on the bf16 data path
    (lstm_fwd_wide16_kernel / lstm_bwd_wide16_kernel, whatever the tile count) -- Hd a multiple of 64; anything else is AIR_E_SHAPE"""
    return bool(M > 0 and Hd > 0 and Hd % 64 == 0)


GAUSS_FOLD_MAX_TILES = 1000     # air_gemm_grouped_gauss_bwd


def latency_form(descs, enabled=True, min_m=4096):
    """the tile form a latency-regime grouped launch (air_gemm_grouped below the wide-tile regime, air_gemm_grouped_opt,
    air_gemm_grouped_gauss_bwd) runs `descs` on: "shortk" (every problem on the streaming body), "shortk_mixed", or (MT, NT, KW) =
    (1, 1, 16) / (1, 1, 4) / (2, 2, 4), the template arguments of gemm_body"""
    mask = shortk_mask(descs, enabled, min_m)
    if mask:
        return "shortk" if mask == (1 << len(descs)) - 1 else "shortk_mixed"
    if group_long_k(descs):
        return (1, 1, 16)
    return (1, 1, 4) if latency_tile(sum(tiles16(d) for d in descs)) == 16 else (2, 2, 4)


def gather_fits(descs, obs, item_floats, B, dataset=0, wide_min_tiles=1000):
    """gemm_kernels.hip air_gemm_grouped_gather_fits: every A a 16-byte aligned column window of obs[B, item_floats] of an fp32 NN / NT
    problem over all B rows, and the group one air_gemm_grouped is sure to run on the 16-wave K-split body (on_long_k_body) -- the body
    the gather launch always runs, so that the product does not depend on which launch carries it"""
    if not (1 <= len(descs) <= 8) or item_floats <= 0 or item_floats % 4 or B <= 0 or obs % 16 or dataset % 16:
        return False
    for d in descs:
        off = (int(d.A) - obs) // 4
        if d.ta or d.A2 or d.C16 or d.precision != 0 or d.M != B or d.lda != item_floats:
            return False
        if (int(d.A) - obs) % 4 or off < 0 or off + d.K > item_floats or off % 4:
            return False
    return on_long_k_body(descs, wide_min_tiles)


def tensors_read(descs, p0, p1, spans):
    """flat-buffer spans (of `spans`, in elements) of the parameter tensors the problems read, the parameters lying at byte
    addresses [p0, p1) (a dX problem reads its layer's weights; weight gradients read activations / gradients only)"""
    out = []
    for d in descs:
        for x in (d.A, d.B, d.aux, d.bias, d.A2):
            if p0 <= int(x or 0) < p1:
                off = (int(x) - p0) // 4
                out += [sp for sp in spans if sp[0] <= off < sp[1]]
    return out


def foldable(descs, g0, r_lo, barred):
    """(mask, covered spans) of the weight-gradient problems that write whole tensors of the head [0, r_lo) of the flat gradient
    buffer (byte address g0) and whose parameters nothing in `barred` reads"""
    mask, cov = 0, []
    for i, d in enumerate(descs):
        if not is_weight_gradient(d):
            continue
        off = (int(d.C) - g0) // 4
        if not (0 <= off < r_lo) or d.ldc != d.N or d.beta != 0.0 or d.epilogue != 0:
            continue
        mine = [(off, off + d.M * d.N)]
        if d.colsum:
            coff = (int(d.colsum) - g0) // 4
            mine.append((coff, coff + d.N))
        if any(a0 < b1 and b0 < a1 for a0, a1 in mine for b0, b1 in barred):
            continue
        mask |= 1 << i
        cov += mine
    return mask, cov


# ---- the whole dispatch rule: which kernel carries a launch ------------------------------------------------------------------------
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -5                      # include/air_hip.h AIR_E_*
FORM_FIELDS = tuple(n for n, _ in _lib.AirGemmForm._fields_)


def _form(**kw):
    f = dict.fromkeys(FORM_FIELDS, 0)
    f.update({k: int(v) for k, v in kw.items()})
    return f


def _cdiv(a, b):
    return (a + b - 1) // b


def _a(p):
    return int(p or 0)


def single_form(M, N, K, colsum=False, ws_bytes=0):
    """gemm_kernels.hip gemm_single_form (air_gemm_form): the kernel of air_gemm / air_gemm_bf16 -- gemm_f32_mfma_kernel<2, 2, 1> from 2048
    32x32 tiles, else <1, 1, 4> with a cross-workgroup K split S (no colsum, a workspace, at least 64 chunks of 16: about 1024 workgroups,
    at least 16 chunks per split, what the workspace holds, at most 16; empty tail splits dropped) -> (status, form)"""
    if M <= 0 or N <= 0 or K <= 0:
        return E_SHAPE, None
    chunks = _cdiv(K, 16)
    if _cdiv(M, 32) * _cdiv(N, 32) >= 2048:
        return 0, _form(family=0, MT=2, NT=2, KW=1, tile=32, S=1, chunks_per_split=chunks, workgroups=_cdiv(M, 32) * _cdiv(N, 128), threads=256)
    tiles = _cdiv(M, 16) * _cdiv(N, 16)
    S = 1
    if not colsum and ws_bytes > 0 and chunks >= 64:
        s = min(1024 // tiles, chunks // 16, ws_bytes // (M * N * 4), 16)
        if s >= 2:
            S = s
    cps = _cdiv(chunks, S)
    return 0, _form(family=0, MT=1, NT=1, KW=4, tile=16, S=_cdiv(chunks, cps), chunks_per_split=cps, workgroups=tiles, threads=256)


def _desc_status(d):
    """gemm_kernels.hip fill_gemm_args: what every grouped entry refuses of one problem"""
    if not (_a(d.A) and _a(d.B) and _a(d.C)):
        return E_NULL
    if not (d.M > 0 and d.N > 0 and d.K > 0):
        return E_SHAPE
    if not (d.lda >= (d.M if d.ta else d.K) and d.ldb >= (d.K if d.tb else d.N) and d.ldc >= d.N):
        return E_SHAPE
    if not 0 <= d.epilogue <= 5:
        return E_UNSUPPORTED
    if d.epilogue in (1, 2) and not _a(d.bias):
        return E_NULL
    if d.epilogue >= 3 and not (_a(d.aux) and d.ldaux >= d.N):
        return E_NULL
    if _a(d.colsum) and not d.ta:
        return E_UNSUPPORTED
    if _a(d.A2):
        if d.ta or not _a(d.a_bias) or d.K % 16 or d.lda % 4:
            return E_UNSUPPORTED
        if _a(d.A) % 16 or _a(d.A2) % 16 or _a(d.a_bias) % 16 or _a(d.a_out) % 16:
            return E_ALIGN
    return 0


def _mirror_usable(m16, ld):
    """gemm_kernels.hip mirror_usable: a bf16 mirror whose rows are 4-byte aligned"""
    return bool(_a(m16) and ld % 2 == 0 and _a(m16) % 4 == 0)


def _big_tn_form(descs, bf16_storage, big_xcd):
    """gemm_kernels.hip big_tn_form: up to 24 problems, the TN ones with 16-byte B rows and M, N, K multiples of 4 on 64x64 tiles (at least
    one), the rest (small_mask) on 16x16 tiles of the same grid; per-problem mirror kinds with bf16 operands"""
    if len(descs) > 24:
        return E_SHAPE, None
    bf = descs[0].precision == 1
    f = _form(grouped=1, MT=4, KW=8, bf=bf, ta=1, threads=512)
    min_k, n_wide = 1 << 30, 0
    for i, d in enumerate(descs):
        if d.precision not in (0, 1) or (d.precision == 1) != bf or _a(d.A2):
            return E_UNSUPPORTED, None
        st = _desc_status(d)
        if st:
            return st, None
        if (d.ta and not d.tb and _a(d.B) % 16 == 0 and d.ldb % 4 == 0 and d.K % 4 == 0 and d.M >= 4 and d.N >= 4 and d.M % 4 == 0
                and d.N % 4 == 0):
            min_k, n_wide = min(min_k, d.K), n_wide + 1
            f["workgroups"] += _cdiv(d.M, 64) * _cdiv(d.N, 64)
        else:
            f["small_mask"] |= 1 << i
            f["workgroups"] += _cdiv(d.M, 16) * _cdiv(d.N, 16)
        if bf and bf16_storage and _mirror_usable(d.A16, d.lda):
            f["a16_mask"] |= 1 << i
        if bf and bf16_storage and _mirror_usable(d.B16, d.ldb):
            f["b16_mask"] |= 1 << i
    if not n_wide:
        return E_UNSUPPORTED, None
    f["xcd_map"] = ((2 if bf else 1) if (big_xcd and min_k >= 1024) else 0)
    f["family"] = 7 if bf else 6
    return 0, f


def wide_group_eligible(descs, bf, wide_min_tiles=1000, wide_tn_bf16=48, wide_tn_f32=48, wide_nt_k=512):
    """gemm_kernels.hip wide_group_eligible, the full rule -> (ok, min K, nt_short): more than `wide_min_tiles` 16x16 tiles, one layout
    (not TT), no A prologue, B 16-byte aligned with ldb % 4 == 0, K % 4 == 0 unless NN, M, N, K >= 4, whole groups of 4 rows / columns of
    an interleaved operand; up to 2048 tiles also A aligned, lda % 4 == 0, K % 4 == 0; TN: at least wide_tn 64x64 tiles and K >= 256;
    NT below K = wide_nt_k: bf16 and more than 2048 tiles only"""
    t16 = sum(tiles16(d) for d in descs)
    ok = t16 > wide_min_tiles
    ta, tb = bool(descs[0].ta), bool(descs[0].tb)
    tiles64, min_k = 0, 1 << 30
    for d in descs:
        if not ok:
            break
        ok = bool(d.ta) == ta and bool(d.tb) == tb and not (ta and tb) and not _a(d.A2)
        ok = ok and _a(d.B) % 16 == 0 and d.ldb % 4 == 0 and (not ta or d.K % 4 == 0) and (not tb or d.K % 4 == 0)
        ok = ok and d.M >= 4 and d.N >= 4 and d.K >= 4 and (not ta or d.M % 4 == 0) and (tb or d.N % 4 == 0)
        if t16 <= 2048:
            ok = ok and _a(d.A) % 16 == 0 and d.lda % 4 == 0 and d.K % 4 == 0
        tiles64 += _cdiv(d.M, 64) * _cdiv(d.N, 64)
        min_k = min(min_k, d.K)
    if ok and ta:
        ok = tiles64 >= (wide_tn_bf16 if bf else wide_tn_f32) and min_k >= 256
    nt_short = (not ta) and tb and min_k < wide_nt_k
    if ok and nt_short:
        ok = bf and t16 > 2048
    return bool(ok), min_k, bool(nt_short)


def longk_half_tile(descs, bf, cus=256, adopted=True):
    """gemm_kernels.hip longk_half_shapes with AIR_GEMM_LONGK_TILE on auto, for a launch on the 16-wave K split of the tile family: the
    (rows, columns) of a 16x16 MFMA tile a workgroup owns -- half tiles (gemm_grouped_longk_half_kernel) for an fp32 GROUP of NT products
    without colsum whose epilogues are NONE / MUL_DELU and whose 16x16 tiling leaves at least half of the `cus` CUs without a tile:
    (8, 16); (16, 16) everywhere else"""
    t16 = sum(tiles16(d) for d in descs)
    domain = not bf and all((not d.ta) and d.tb and not _a(d.colsum) and d.epilogue in (0, 3) for d in descs)
    return (8, 16) if (adopted and domain and len(descs) > 1 and 2 * t16 <= cus) else (16, 16)


def grouped_form(descs, wide_min_tiles=1000, shortk=True, shortk_min_m=4096, shortk_wgs=384, wide_tn_bf16=48, wide_tn_f32=48, wide_nt_k=512,
                 bf16_storage=True, big_xcd=True, cus=256):
    """gemm_kernels.hip gemm_grouped_form (air_gemm_grouped_form): the whole rule of air_gemm_grouped -> (status, form | None), the form a
    dict over the fields of AirGemmForm.  The keyword arguments are the library's environment-tunable thresholds at their defaults
    (AIR_GEMM_WIDE_MIN_TILES, AIR_GEMM_SHORTK, AIR_GEMM_SHORTK_MIN_M, AIR_GEMM_SHORTK_WGS, AIR_GEMM_WIDE_TN_BF16, AIR_GEMM_WIDE_TN_F32,
    AIR_GEMM_WIDE_NT_K, AIR_GEMM_BF16_STORAGE, AIR_GEMM_BIG_XCD).  In order: more than 8 problems -> the big TN group; a plain fp32 group
    with streaming short-K weight gradients -> "shortk"; the wide-tile regime (bf16 TN: the big-group launch, per-problem mirrors);
    else the tile families "c16" / "apro" / "tile" on <1, 1, 16> (group_long_k), <1, 1, 4> or <2, 2, 4>; a "tile" launch on <1, 1, 16>
    may run on half tiles (longk_half_tile: small_mask = its problems, workgroups = the half tiles; `cus` = the device's CUs)."""
    count = len(descs)
    if count > 8:
        return _big_tn_form(descs, bf16_storage, big_xcd)
    if count <= 0:
        return E_SHAPE, None

    def validate():
        for d in descs:
            st = _desc_status(d)
            if st:
                return st
        return 0

    skm = 0
    if shortk and not any(_a(d.A2) or _a(d.C16) or d.precision != 0 for d in descs):
        skm = sum(1 << i for i, d in enumerate(descs) if shortk_eligible(d, shortk_min_m))
    if skm:
        st = validate()
        if st:
            return st, None
        tile = latency_tile(sum(tiles16(d) for i, d in enumerate(descs) if not (skm >> i) & 1))
        wgs = sum(shortk_workgroups(d.M, shortk_wgs) if (skm >> i) & 1 else _cdiv(d.M, tile) * _cdiv(d.N, tile) for i, d in enumerate(descs))
        return 0, _form(family=3, grouped=1, sk_mask=skm, tile=tile, MT=tile // 16, NT=tile // 16, KW=4, threads=256, workgroups=wgs)
    t16 = sum(tiles16(d) for d in descs)
    tile = latency_tile(t16)
    st = validate()
    if st:
        return st, None
    lk = group_long_k(descs)
    bf = descs[0].precision == 1
    if any(d.precision not in (0, 1) or (d.precision == 1) != bf for d in descs):
        return E_UNSUPPORTED, None
    ok, min_k, nt_short = wide_group_eligible(descs, bf, wide_min_tiles, wide_tn_bf16, wide_tn_f32, wide_nt_k)
    ta, tb = bool(descs[0].ta), bool(descs[0].tb)
    if ok and bf and ta:
        return _big_tn_form(descs, bf16_storage, big_xcd)
    if ok:
        MT = 4 if ta else (2 if nt_short else 1)
        f = _form(family=5 if bf else 4, grouped=count > 1, bf=bf, ta=ta, tb=tb, nt_short=nt_short, MT=MT, KW=8, threads=512,
                  workgroups=sum(_cdiv(d.M, 16 * MT) * _cdiv(d.N, 64) for d in descs), xcd_map=ta and min_k >= 1024)
        if bf:
            full = (1 << count) - 1
            f["a16_mask"] = full if bf16_storage and all(_mirror_usable(d.A16, d.lda) for d in descs) else 0
            f["b16_mask"] = full if bf16_storage and all(_mirror_usable(d.B16, d.ldb) for d in descs) else 0
        return 0, f
    if any(_a(d.A2) for d in descs) and count != 1:
        return E_UNSUPPORTED, None
    mt = 1 if (lk or tile == 16) else 2
    f = _form(grouped=count > 1, bf=bf, tile=tile, long_k=lk, MT=mt, NT=mt, KW=16 if lk else 4, threads=1024 if lk else 256,
              workgroups=sum(_cdiv(d.M, tile) * _cdiv(d.N, tile) for d in descs))
    if any(_a(d.C16) for d in descs):
        if not bf or _a(descs[0].A2):
            return E_UNSUPPORTED, None
        f["family"] = 1
    elif count == 1 and _a(descs[0].A2):
        if tile != 16:
            return E_UNSUPPORTED, None
        f.update(family=2, MT=1, NT=1, KW=4, threads=256)
    elif lk:
        tr, tc = longk_half_tile(descs, bf, cus)
        if (tr, tc) != (16, 16):
            f.update(grouped=1, small_mask=(1 << count) - 1, workgroups=sum(_cdiv(d.M, tr) * _cdiv(d.N, tc) for d in descs))
    return 0, f
