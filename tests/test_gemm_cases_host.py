"""Host checks of tests/gemm_cases.py (no GPU): every row of the case table against the Python mirror of the GEMM dispatch
(gemm_groups.grouped_form / single_form) AND the library's own host-only queries (air_gemm_grouped_form / air_gemm_form); a row for
every kernel the launch switches can reach; a seeded sweep of random descriptor groups, mirror against library, field for field; the
float32 restatement of every comparison within RESTATEMENT_SHARE of its bound; every planted defect at least DEFECT_MARGIN bounds
away from the float64 reference.

The defects, applied to the float64 reference of every problem they apply to:
  k_last / k_tail   one k-term dropped, in the last full 16-chunk and in the K tail
  cols / rows       two neighbouring output columns / rows swapped at the edge of the first 16 x 16 tile
  round_f32         precision 0 computed from bf16-rounded operands;  round_bf16: precision 1 computed from unrounded operands
  bias_last         the bias of the last column omitted;  beta: beta ignored;  delu_row: ELU' taken from the next aux row
  colsum_a          colsum summed over op(A) instead of B
A defect that moves the accumulator by a known amount (k_last, k_tail, bias_last, beta) must exceed the bound 4 x at EVERY element it
touches through which the epilogue passes at least half of a change (ELU' >= 0.5: a saturated ELU hides any accumulator from any
test), and those are at least a quarter of the touched elements.  The others change an element by a random amount, which can be small
at single elements whatever the bound: they must exceed the bound 4 x at half of the touched elements at least (the rounding defects: of
the touched elements the epilogue passes)."""
import ctypes
import functools
import random

import pytest
import torch

import gemm_cases as GC
from attend_infer_repeat_amd import _lib, gemm_groups as GG
from gemm_cases import BF16, F32

NAMES = list(GC.CASES)


@pytest.fixture(scope="module")
def lib():
    from attend_infer_repeat_amd import build
    build.build()
    return _lib.load()


def _lib_grouped(lib, descs):
    arr = (_lib.AirGemmDesc * len(descs))(*descs)
    f = _lib.AirGemmForm()
    st = lib.air_gemm_grouped_form(arr, len(descs), ctypes.byref(f))
    return st, (f.as_dict() if st == 0 else None)


def _forms(lib, name):
    """[(expected fields, mirror, library)] per product the row launches: one, or the two of air_linear_bwd"""
    case = GC.CASES[name]
    if case["entry"] == "grouped":
        ds = GC.descs(name)
        return [(case["form"], GG.grouped_form(ds), _lib_grouped(lib, ds))]
    ws = (64 << 20) if case["ws"] is None else case["ws"]
    want = case["form"] if isinstance(case["form"], list) else [case["form"]]
    assert len(want) == len(case["problems"])
    out = []
    for w, pr in zip(want, case["problems"]):
        f = _lib.AirGemmForm()
        st = lib.air_gemm_form(pr["M"], pr["N"], pr["K"], int(pr["colsum"]), ws, ctypes.byref(f))
        out.append((w, GG.single_form(pr["M"], pr["N"], pr["K"], pr["colsum"], ws), (st, f.as_dict())))
    return out


def _row_keys(lib, names):
    keys = set()
    for name in names:
        case = GC.CASES[name]
        for _, (st, f), _ in _forms(lib, name):
            assert st == 0, name
            keys.add(GC.form_key(case["entry"], case["precision"], dict(f, family=_lib.GEMM_FAMILIES[f["family"]])))
    return keys


def test_every_row_runs_on_the_kernel_it_names(lib):
    for name in NAMES:
        for want, (st_m, fm), (st_l, fl) in _forms(lib, name):
            assert st_m == 0 and st_l == 0, (name, st_m, st_l)
            assert fm == fl, (name, {k: (fm[k], fl[k]) for k in fm if fm[k] != fl[k]})
            want = dict(want, family=_lib.GEMM_FAMILIES.index(want["family"]))
            got = {k: fm[k] for k in want}
            assert got == want, (name, got, want)


def test_every_reachable_kernel_has_a_row(lib):
    reach = GC.reachable()
    have = _row_keys(lib, NAMES)
    assert not (reach - have), sorted(reach - have, key=str)
    assert not (have - reach), sorted(have - reach, key=str)          # a row on a kernel the enumeration does not know
    # the check bites: without the rows of one kernel, that kernel is reported
    for gone in ("gemm_bf16_kw1_", "wide16_nts_a1b0_lone", "grouped_shortk_tile32", "big_f32_", "linear_bwd_kw1"):
        left = [n for n in NAMES if not n.startswith(gone)]
        assert len(left) < len(NAMES)
        assert reach - _row_keys(lib, left), gone


def _random_group(rng):
    """a random descriptor group around one of the regimes of the dispatch (pointers are integers).  A clean group keeps what the
    regime's kernels ask for -- whole float4 rows, 16-byte starts, one precision, valid epilogues --, the others are perturbed in every
    field the rule reads: odd leading dimensions, unaligned starts, mixed layouts and precisions, A2 / C16 / A16 / B16, NULL pointers"""
    regime = rng.choice(["tile", "long_k", "tile32", "wide", "wide", "wide_far", "big", "shortk", "apro", "any"])
    clean = rng.random() < 0.6
    count = 1 if regime == "apro" else rng.randint(1, 8)
    if regime == "big":
        count = rng.randint(9, 25 if rng.random() < 0.05 else 24)
    layout = rng.choice(GC.LAYOUTS[:3])
    prec = rng.choice([0, 0, 1])
    wide = regime in ("wide", "wide_far", "big")
    descs = []
    for i in range(count):
        ta, tb = layout if (wide and (clean or rng.random() < 0.9)) else rng.choice(GC.LAYOUTS)
        if regime == "big":
            ta, tb = (1, 0) if rng.random() < 0.9 else rng.choice(GC.LAYOUTS)
        if regime in ("tile", "apro"):
            M, N, K = rng.randint(1, 70), rng.randint(1, 70), rng.randint(1, 600)
            if regime == "apro":
                ta, K = 0, rng.choice([16, 64, 512, 520, 24])
        elif regime == "long_k":
            M, N, K = rng.randint(1, 64), rng.randint(1, 300), rng.choice([511, 512, 520, 1024, 2500])
        elif regime == "tile32":
            M, N, K = rng.randint(100, 400), rng.randint(100, 400), rng.randint(1, 64)
        elif regime in ("wide", "wide_far"):
            per = rng.choice([900, 1100, 1500]) * (1 if regime == "wide" else 2) // count + 1       # 16 x 16 tiles per problem
            mt = rng.randint(2, 12)
            M, N = 16 * mt - 4 * rng.randint(0, 3), 16 * (per // mt + 1) - 4 * rng.randint(0, 3)
            K = rng.choice([4, 12, 16, 20, 50, 256, 260, 508, 512, 1024, 1028])
            if ta and rng.random() < 0.7:
                K = rng.choice([256, 260, 1024, 1028])
        elif regime == "big":
            M, N, K = rng.choice([1, 2, 3, 50, 64, 68, 128]), rng.choice([1, 6, 64, 72, 256]), rng.choice([5, 33, 256, 1024, 1028])
        elif regime == "shortk":
            M, N, K = rng.choice([37, 4095, 4096, 4100, 6163]), rng.choice([20, 64, 128, 192, 256, 320]), rng.choice([16, 32, 48, 64, 80, 24])
            ta, tb = (1, 0) if rng.random() < 0.8 else rng.choice(GC.LAYOUTS)
            if rng.random() < 0.3:
                M, N, K = 810, 500, 24                   # more than 1536 tiles beside the streaming problems: 32 x 32 tiles
        else:
            M, N, K = rng.randint(1, 3000), rng.randint(1, 3000), rng.randint(1, 3000)
        if not clean and rng.random() < 0.15:
            M += rng.randint(-3, 3); N += rng.randint(-3, 3); K += rng.randint(-3, 3)
            M, N, K = max(M, 0), max(N, 0), max(K, 0)
        odd = lambda: rng.choice([0, 4, 8]) if clean else (rng.choice([0, 0, 0, 1, 2, 3, 4, 8]) if rng.random() < 0.5 else 0)
        start = lambda: (1 << 24) * rng.randint(1, 200) + (rng.choice([0, 16, 32]) if clean else rng.choice([0, 0, 0, 0, 2, 4, 8, 16, 32]))
        null = lambda p: not clean and rng.random() < p
        lda, ldb, ldc = (M if ta else K) + odd(), (K if tb else N) + odd(), N + odd()
        if null(0.03):
            lda -= 1
        epi = rng.choice([0, 0, 0, 1, 2, 3, 4, 5]) if not null(0.02) else 6
        beta = rng.choice([0.0, 0.0, 0.5])
        if regime == "shortk" and clean:
            epi, beta = 0, 0.0
        d = _lib.AirGemmDesc(ta, tb, M, N, K, None if null(0.01) else start(), lda, start(), ldb, start(), ldc,
                             start() if (epi in (1, 2) and not null(0.03)) or (epi >= 4 and rng.random() < 0.3) else None, epi,
                             start() if (epi >= 3 and not null(0.03)) else None, N + odd() - (1 if null(0.02) else 0),
                             beta, start() if (rng.random() < (0.4 if ta else (0.0 if clean else 0.02))) else None,
                             rng.choice([0, 1, 2]) if null(0.03) else prec, None, None, 0, None)
        if regime == "apro" or null(0.02):
            d.A2, d.a_bias, d.a_elu, d.a_out = start(), (None if null(0.05) else start()), rng.randint(0, 1), rng.choice([None, start()])
        if rng.random() < 0.25:
            d.A16 = start()
        if rng.random() < 0.25:
            d.B16 = start()
        if rng.random() < (0.15 if not clean or prec else 0.0):
            d.C16 = start()
        descs.append(d)
    if wide and rng.random() < 0.5:                             # mirrors for the whole launch, usable or not
        for d in descs:
            d.A16, d.B16 = (1 << 30) + rng.choice([0, 0, 0, 2]), (1 << 31) + 4
    return descs


def test_mirror_matches_library_on_random_groups(lib):
    rng = random.Random(20251019)
    seen, statuses = {}, {}
    for trial in range(6000):
        descs = _random_group(rng)
        (st_m, fm), (st_l, fl) = GG.grouped_form(descs), _lib_grouped(lib, descs)
        what = [(d.ta, d.tb, d.M, d.N, d.K, d.lda, d.ldb, d.precision) for d in descs]
        assert st_m == st_l, (trial, st_m, st_l, what)
        statuses[st_l] = statuses.get(st_l, 0) + 1
        if st_l == 0:
            assert fm == fl, (trial, {k: (fm[k], fl[k]) for k in fm if fm[k] != fl[k]}, what)
            key = (fl["family"], fl["grouped"], fl["MT"], fl["KW"], fl["bf"], fl["ta"], fl["tb"], int(fl["a16_mask"] != 0), int(fl["b16_mask"] != 0))
            seen[key] = seen.get(key, 0) + 1
    # the sweep reaches every family, lone and grouped, and every refusal
    assert {k[0] for k in seen} == set(range(8)), sorted(seen)
    assert set(statuses) >= {0, GG.E_NULL, GG.E_SHAPE, GG.E_ALIGN, GG.E_UNSUPPORTED}, statuses
    lone_and_grouped = {(k[0], k[1]) for k in seen}
    assert lone_and_grouped >= {(f, g) for f in (0, 1, 4, 5) for g in (0, 1)} | {(2, 0), (3, 1), (6, 1), (7, 1)}, sorted(lone_and_grouped)
    print(f"\n[gemm cases] sweep: {len(seen)} distinct kernels, statuses {statuses}")
    assert len(seen) >= 40, sorted(seen)
    for trial in range(3000):
        M, N, K = rng.randint(1, 2100), rng.randint(1, 2100), rng.choice([rng.randint(1, 100), rng.randint(1000, 5000)])
        colsum, ws = rng.random() < 0.3, rng.choice([0, 0, 64 << 20, rng.randint(0, 1 << 22)])
        f = _lib.AirGemmForm()
        assert lib.air_gemm_form(M, N, K, int(colsum), ws, ctypes.byref(f)) == 0
        assert GG.single_form(M, N, K, colsum, ws) == (0, f.as_dict()), (M, N, K, colsum, ws)
    assert lib.air_gemm_form(0, 4, 4, 0, 0, ctypes.byref(_lib.AirGemmForm())) == GG.single_form(0, 4, 4)[0] == GG.E_SHAPE


# ---------------------------------------------------------------------------------------------------------------
# the restatement's share of every bound, and the margins of the planted defects
# ---------------------------------------------------------------------------------------------------------------
def _ratios(diff, bnd):
    return (diff.abs() / bnd).reshape(-1)


def _everywhere(ratio, passing):
    """a defect of known size: 4 bounds at every touched element the epilogue lets half of a change through; >= a quarter of them"""
    passing = passing.reshape(-1)
    assert int(passing.sum()) * 4 >= passing.numel() or (passing.numel() < 64 and bool(passing.any()))      # (a short column: one at least)
    return float(ratio[passing].min())


def _at_half(ratio):
    """a defect of random size: the margin at the median touched element"""
    return float(ratio.double().median())


def _gain(pr, d):
    """d out / d acc of the epilogue at the float64 reference"""
    if pr["epi"] == GC.EPI_MUL_DELU:
        return GC.elu_prime(d["aux"].v.double())
    if pr["epi"] in (GC.EPI_BIAS_ELU, GC.EPI_ADD_AUX_ELU):
        return torch.where(d["out64"] > 0, torch.ones_like(d["out64"]), d["out64"] + 1)
    return torch.ones_like(d["out64"])


@functools.lru_cache(maxsize=None)
def _analyse(name):
    """-> (worst restatement share, {defect: smallest margin over the problems it applies to})"""
    case, share, margins = GC.CASES[name], 0.0, {}

    def note(defect, m):
        margins[defect] = min(margins.get(defect, float("inf")), m)

    r16 = GC._rounded(BF16)
    for pr, d in zip(case["problems"], GC.data(name)):
        bnd, out64, acc = GC.bound(case, d), d["out64"], d["acc64"]
        out32, cs32 = GC.restate32(case, pr, d)
        share = max(share, float(_ratios(out32.double() - out64, bnd).max()))
        if cs32 is not None:
            share = max(share, float(_ratios(cs32.double() - d["colsum64"], GC.colsum_bound(case, d)).max()))
        a32, b32 = GC.op_a32(pr, d), (d["B"].v.t() if pr["tb"] else d["B"].v)
        r = GC._rounded(case["precision"])
        a64, b64 = r(a32).double(), r(b32).double()
        passing = _gain(pr, d) >= 0.5
        defect = lambda acc_d, **kw: GC.epilogue(acc_d, dict(pr, **kw), d) - out64
        K, M, N = pr["K"], pr["M"], pr["N"]
        for tag, k in (("k_last", K // 16 * 16 - 1), ("k_tail", K - 1 if K % 16 else -1)):
            if k >= 0:
                note(tag, _everywhere(_ratios(defect(acc - a64[:, k:k + 1] * b64[k:k + 1, :]), bnd), passing))
        for tag, dim, n in (("cols", 1, N), ("rows", 0, M)):
            if n >= 2:
                i0 = min(15, n - 2)
                idx = torch.arange(n)
                idx[i0], idx[i0 + 1] = i0 + 1, i0
                sw = out64.index_select(dim, idx) - out64
                note(tag, _at_half(_ratios(sw.narrow(dim, i0, 2), bnd.narrow(dim, i0, 2))))
        other = (r16(a32).double() @ r16(b32).double()) if case["precision"] == F32 else (a32.double() @ b32.double())
        note("round_f32" if case["precision"] == F32 else "round_bf16", _at_half(_ratios(defect(other), bnd)[passing.reshape(-1)]))
        if pr["bias"]:
            sav = d["bias"].parent.clone()
            d["bias"].v[0, N - 1] = 0.0
            dd = (GC.epilogue(acc, pr, d) - out64)[:, N - 1]
            d["bias"].parent.copy_(sav)
            note("bias_last", _everywhere(_ratios(dd, bnd[:, N - 1]), passing[:, N - 1]))
        if pr["beta"] != 0.0:
            note("beta", _everywhere(_ratios(defect(acc, beta=0.0), bnd), passing))
        if pr["epi"] == GC.EPI_MUL_DELU and M >= 2:
            g = GC.elu_prime(d["aux"].v.double())
            note("delu_row", _at_half(_ratios(acc * (torch.roll(g, -1, 0) - g) + (pr["beta"] * d["C0"].v.double() * (torch.roll(g, -1, 0) - g)
                                                                                  if pr["beta"] else 0.0), bnd)))
        if pr["colsum"]:
            n = min(M, N)
            note("colsum_a", _at_half(_ratios(a32.double().sum(1)[:n] - d["colsum64"][:n], GC.colsum_bound(case, d)[:n])))
    return share, margins


def test_restatement_stays_within_its_share_of_every_bound():
    worst = {}
    for name in NAMES:
        share, _ = _analyse(name)
        grp = GC.CASES[name]["group"]
        if share > worst.get(grp, (0.0, ""))[0]:
            worst[grp] = (share, name)
        assert share <= GC.RESTATEMENT_SHARE, (name, share)
    for grp in sorted(worst):
        print(f"\n[gemm cases] group {grp}: worst float32 restatement share of the bound {worst[grp][0]:.3g} ({worst[grp][1]})")
    assert sorted(worst) == sorted(GC.CONST)


def test_every_planted_defect_clears_the_bound():
    worst, applied = {}, set()
    for name in NAMES:
        _, margins = _analyse(name)
        for defect, m in margins.items():
            applied.add(defect)
            if m < worst.get(defect, (float("inf"), ""))[0]:
                worst[defect] = (m, name)
            assert m >= GC.DEFECT_MARGIN, (name, defect, m)
    assert applied == {"k_last", "k_tail", "cols", "rows", "round_f32", "round_bf16", "bias_last", "beta", "delu_row", "colsum_a"}
    for defect in sorted(worst):
        print(f"\n[gemm cases] defect {defect}: smallest margin {worst[defect][0]:.3g} bounds ({worst[defect][1]})")


def test_cases_keep_their_promises():
    """what the comparisons rely on, at the cheap rows: magnitudes, NaN parents, alignment as asked"""
    for name in NAMES:
        case = GC.CASES[name]
        if sum(p["M"] * p["N"] for p in case["problems"]) > 100000:
            continue
        for pr, d in zip(case["problems"], GC.data(name)):
            for k in ("A", "B"):
                v = d[k]
                assert bool(((v.v.abs() >= 0.5 - 1e-6) & (v.v.abs() <= 1.5 + 1e-6)).all())
                assert bool(torch.isnan(v.outside(v.parent)).all()) and v.lead >= 2 * v.ld
                assert v.lead % 4 == pr["a_un" if k == "A" else "b_un"]
            assert pr["apro"] or bool((d["S"] >= 0.25 * pr["K"] * (1 - 2 ** -7)).all())
