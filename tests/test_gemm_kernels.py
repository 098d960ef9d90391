"""GPU parity of the GEMM family, one launch at a time (run with -m gpu on an MI355X): air_gemm, air_gemm_bf16, air_linear_fwd /
air_linear_bwd and air_gemm_grouped on every kernel their launch switches can reach.  Cases, float64 references and bounds come from
tests/gemm_cases.py; tests/test_gemm_cases_host.py holds every case against the dispatch rule on the CPU, sets the bound's constants
from a float32 restatement and checks that the planted defects clear the bound.

Per case: one launch, status 0; every output element within its bound of float64; no NaN left inside an output view (every one starts
as NaN); every parent's padding bit-equal to the sentinel it was filled with, every input parent (NaN outside its view) unchanged;
C16 exactly bf16(C).  Group letters (R single entries, S tile families of air_gemm_grouped, T wide-tile kernels, U big group) tag
every comparison, "16" appended for precision 1 (the same bound and constant: the report keeps the bf16 MFMA's figure apart); the
worst error / bound ratio of each is printed when the module finishes (pytest -s).

Bit for bit, with no tolerance: a problem alone and in each slot 0..7 of a group on the same body; a lone air_gemm_grouped problem
against air_gemm without workspace where both run gemm_f32_mfma_kernel<1, 1, 4>; rows of op(A) / columns of op(B) reversed against
rows / columns of C reversed; the four A16 / B16 mirror combinations; precision 1 on A against precision 1 on bf16(A).

Reversal on shortk_dw_body: the streaming body keeps ONE accumulation chain per element in a fixed k order (no LDS reduction, no K
split; csrc/gemm_kernels.hip shortk_dw_body), so an element's K order does not depend on its slab or column quarter: the code gives
the same guarantee as the tile bodies, and test_rows_and_columns_reversed holds it there too.

Worst error / bound on an MI355X (the float32 restatement on the CPU: 0.199 / 0.209 / 0.196 / 0.226 of the bound): fp32 operands R 0.212 (the dx product of
air_linear_bwd),
S 0.215, T 0.233, U 0.101; bf16 operands R 0.096, S 0.085, T 0.077, U 0.042 -- the bf16 MFMAs' internal summation stays inside the
share the fp32 restatement leaves, and well inside the fp32 chains' own figure (the products of bf16 operands are exact).

One kernel bug surfaced with these tests: the colsum of gemm_wide16_body<TN, A16, B16> (two 32-deep chunks in flight per wave) counted
the last chunk again for every wave whose second chunk fell past the end, whenever K / 32 is no multiple of 16 (K = 256, 768: the rows
big_bf16_14, big_bf16_handover, big_bf16_9_k768 were off by whole terms).  Fixed in csrc/gemm_kernels.hip."""
import pytest
import torch

import fold_cases as FC
import gemm_cases as GC
from fold_cases import SENTINEL, assert_bits, print_worst
from gemm_cases import BF16, F32, NAN, View, _lead

pytestmark = pytest.mark.gpu
NAMES = list(GC.CASES)
SENT16 = float(torch.tensor(SENTINEL).to(torch.bfloat16))
TILE_BODY = ("family", "MT", "NT", "KW", "bf", "ta", "tb")


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print_worst("gemm kernels", [g + p for g in "RSTU" for p in ("", "16")])


def within(out, ref64, bnd, what, group):
    """|out - ref64| <= bnd for every element, none left out; the worst ratio goes to the group's report"""
    out = out.detach().cpu().double()
    assert out.shape == ref64.shape, f"{what}: shape {tuple(out.shape)} against {tuple(ref64.shape)}"
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} elements not finite (an output left unwritten?)"
    ratio = (out - ref64).abs() / bnd
    worst = float(ratio.max())
    if group is not None and (group not in FC.WORST or worst > FC.WORST[group][0]):
        FC.WORST[group] = (worst, what)
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3g} at {divmod(int(ratio.argmax()), ratio.shape[-1])}"


def _out(rows, cols, ld, lead, dtype=torch.float32, init=None):
    """an output window of a sentinel-filled parent on the device: NaN inside, or a copy of `init` (a View: the C that beta reads)"""
    v = View(rows, cols, ld, lead, SENT16 if dtype == torch.bfloat16 else SENTINEL, dtype=dtype)
    if init is None:
        v.v.fill_(NAN)
    else:
        v.v.copy_(init.v)
    par = v.parent.cuda()
    return v, par, v.on(par)


def _padding_untouched(v, par, what):
    fill = torch.full((1,), SENT16 if par.dtype == torch.bfloat16 else SENTINEL, dtype=par.dtype)
    pad = v.outside(par)
    assert bool((pad == fill).all()), f"{what}: {int((pad != fill).sum())} elements outside the view written"


def stage(name, mirrors=None, pre_round_a=False):
    """the case on the device: per problem the input windows (parents uploaded whole), the output windows and a problem dict for
    hip.gemm_grouped.  mirrors = (a16, b16) overrides which mirrors are handed over; pre_round_a: A holds bf16(A) already"""
    case, out = GC.CASES[name], []
    for pr, d in zip(case["problems"], GC.data(name)):
        M, N, K = pr["M"], pr["N"], pr["K"]
        s = dict(pr=pr, d=d, inputs={}, outputs={})
        for k in ("A", "B", "A2", "a_bias", "bias", "aux"):
            if k in d:
                host = d[k].parent
                if k == "A" and pre_round_a:
                    host = host.to(torch.bfloat16).float()
                par = host.cuda()
                s["inputs"][k] = (d[k], par, host)
                s[k] = d[k].on(par)
        ldc = N + pr["pads"][2]
        s["outputs"]["C"] = _out(M, N, ldc, _lead(ldc, 0), init=d.get("C0"))
        if pr["colsum"]:
            s["outputs"]["colsum"] = _out(1, N, N, 4)
        if pr["c16"]:
            s["outputs"]["C16"] = _out(M, N, ldc, _lead(ldc, 0), dtype=torch.bfloat16)
        if pr["apro"]:
            s["outputs"]["a_out"] = _out(M, K, d["A"].ld, d["A"].lead)
        a16, b16 = (pr["a16"], pr["b16"]) if mirrors is None else mirrors
        for k, on in (("A", a16), ("B", b16)):
            if on:
                m = GC._mirror(d[k])
                par = m.parent.cuda()
                s["inputs"][k + "16"] = (m, par, m.parent)
                s[k + "16"] = m.on(par)
        o = {k: w for k, (_, _, w) in s["outputs"].items()}
        s["problem"] = dict(A=s["A"], B=s["B"], ta=bool(pr["ta"]), tb=bool(pr["tb"]), epilogue=pr["epi"], beta=pr["beta"], out=o["C"],
                            bias=s["bias"][0] if "bias" in s else None, aux=s.get("aux"), colsum=o["colsum"][0] if pr["colsum"] else None,
                            A16=s.get("A16"), B16=s.get("B16"), C16=o.get("C16"))
        if pr["apro"]:
            s["problem"].update(A2=s["A2"], a_bias=s["a_bias"][0], a_elu=pr["apro"] == "elu", a_out=o["a_out"])
        out.append(s)
    return out


def launch(hip, name, staged):
    case = GC.CASES[name]
    if case["entry"] == "grouped":
        hip.gemm_grouped([s["problem"] for s in staged], precision=case["precision"])
        return
    s = staged[0]
    p, pr = s["problem"], s["pr"]
    if case["entry"] == "gemm":
        hip.gemm(p["A"], p["B"], ta=p["ta"], tb=p["tb"], bias=p["bias"], epilogue=p["epilogue"], aux=p["aux"], beta=p["beta"], out=p["out"],
                 colsum=p["colsum"] if p["colsum"] is not None else False, use_workspace=case["ws"] != 0, precision=case["precision"],
                 ws_bytes=case["ws"])
    elif case["entry"] == "linear_fwd":
        hip.linear_fwd(p["A"], p["B"], p["bias"], hip.ACT_ELU, out=p["out"])
    else:
        # the row's two problems are the products of the one call: dx = dy . w^T (A = dy, B = w), dw = x^T . dy with db (A = x, B = dy)
        dx, dw = staged[0]["problem"], staged[1]["problem"]
        hip.linear_bwd(dw["A"], dx["B"], None, dx["A"], hip.ACT_NONE, out=(dx["out"], dw["out"], dw["colsum"]))


def check(name, staged):
    case = GC.CASES[name]
    for i, s in enumerate(staged):
        pr, d, tag = s["pr"], s["d"], f"{name}[{i}] "
        _, _, C = s["outputs"]["C"]
        grp = case["group"] + ("16" if case["precision"] else "")
        within(C, d["out64"], GC.bound(case, d), tag + "C", grp)
        if pr["colsum"]:
            within(s["outputs"]["colsum"][2][0], d["colsum64"], GC.colsum_bound(case, d), tag + "colsum", grp)
        if pr["c16"]:
            assert_bits(s["outputs"]["C16"][2].contiguous(), C.to(torch.bfloat16).contiguous(), tag + "C16 against bf16(C)")
        if pr["apro"]:
            a_out = s["outputs"]["a_out"][2]
            if pr["apro"] == "lin":
                assert_bits(a_out.contiguous(), d["a32"].contiguous(), tag + "a_out")            # (the sums are exact in float32)
            else:       # a bound of its own (a few units of expf in a float32 sum of three), kept out of the groups' report
                within(a_out, GC.elu64((d["A"].v + d["A2"].v + d["a_bias"].v[0]).double()), 8 * GC.U32 * (d["a32"].double().abs() + 1), tag + "a_out", None)
        for k, (v, par, _) in s["outputs"].items():
            _padding_untouched(v, par, tag + k)
        for k, (v, par, host) in s["inputs"].items():
            same = par.cpu().view(torch.int16 if par.dtype == torch.bfloat16 else torch.int32) == host.view(torch.int16 if par.dtype == torch.bfloat16 else torch.int32)
            assert bool(same.all()), tag + k + ": an input buffer was written"


@pytest.mark.parametrize("name", NAMES)
def test_case_against_float64(hip, name):
    case = GC.CASES[name]
    staged = stage(name)
    if case["entry"] == "grouped":                                # the kernel the row names, asked of the library on the real addresses
        st, f = hip.gemm_grouped_form([s["problem"] for s in staged], precision=case["precision"])
        want = dict(case["form"], family=hip._lib.GEMM_FAMILIES.index(case["form"]["family"]))
        assert st == 0 and {k: f[k] for k in want} == want, (name, st, f)
    launch(hip, name, staged)
    torch.cuda.synchronize()
    check(name, staged)


# ---------------------------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------------------------
def _rand(gen, rows, cols):
    return GC._signed(gen, rows, cols).cuda()


def _plain(gen, ta, tb, M, N, K, **kw):
    """a problem on plain contiguous tensors (16-byte aligned starts)"""
    return dict(A=_rand(gen, K, M) if ta else _rand(gen, M, K), B=_rand(gen, N, K) if tb else _rand(gen, K, N), ta=bool(ta), tb=bool(tb), **kw)


def _body(hip, problems, precision):
    st, f = hip.gemm_grouped_form(problems, precision=precision)
    assert st == 0
    return tuple(f[k] for k in TILE_BODY)


def _fresh(pr):
    M = pr["A"].shape[1] if pr["ta"] else pr["A"].shape[0]
    N = pr["B"].shape[0] if pr["tb"] else pr["B"].shape[1]
    return dict(pr, out=torch.full((M, N), NAN, device="cuda"))


# the problem under test, its fillers, precision: every group of seven fillers + the problem stays on the lone problem's body
SLOT_CASES = {
    "tile16_f32": ((0, 0, 37, 50, 70), (1, 0, 16, 8, 64), F32),
    "tile16_bf16": ((0, 1, 37, 50, 70), (0, 0, 16, 8, 64), BF16),
    "long_k_f32": ((0, 0, 20, 48, 520), (0, 1, 16, 4, 512), F32),
    "tile32_bf16": ((0, 0, 810, 501, 24), (1, 1, 16, 8, 16), BF16),
    "wide_f32_nn": ((0, 0, 126, 2064, 20), (0, 0, 16, 64, 20), F32),
    "wide16_nt": ((0, 1, 125, 2063, 512), (0, 1, 16, 64, 512), BF16),
}


@pytest.mark.parametrize("which", list(SLOT_CASES))
def test_slot_independence(hip, which):
    """a problem alone, and in each slot 0..7 of a group the library keeps on the same body: the same bits"""
    shape, filler, prec = SLOT_CASES[which]
    gen = torch.Generator().manual_seed(31 + len(which))
    X = _plain(gen, *shape)
    fillers = [_plain(gen, *filler) for _ in range(7)]
    lone = _fresh(X)
    body = _body(hip, [lone], prec)
    hip.gemm_grouped([lone], precision=prec)
    for slot in range(8):
        group = [_fresh(f) for f in fillers[:slot]] + [_fresh(X)] + [_fresh(f) for f in fillers[slot:]]
        assert _body(hip, group, prec) == body, (which, slot)
        hip.gemm_grouped(group, precision=prec)
        torch.cuda.synchronize()
        assert_bits(group[slot]["out"], lone["out"], f"{which}: slot {slot} against the lone launch")


@pytest.mark.parametrize("precision", [F32, BF16])
@pytest.mark.parametrize("ta,tb", GC.LAYOUTS)
def test_lone_grouped_against_single_entry(hip, ta, tb, precision):
    """a lone air_gemm_grouped problem against air_gemm / air_gemm_bf16 without workspace: both run gemm_f32_mfma_kernel<1, 1, 4>"""
    gen = torch.Generator().manual_seed(97 + 2 * ta + tb)
    X = _plain(gen, ta, tb, 37, 50, 70, bias=_rand(gen, 1, 50)[0], epilogue=GC.EPI_BIAS_ELU)
    a, b = _fresh(X), _fresh(X)
    st, f = hip.gemm_grouped_form([a], precision=precision)
    g = hip.gemm_form(37, 50, 70, False, 0)
    assert st == 0 and all(f[k] == g[k] for k in ("family", "MT", "NT", "KW", "grouped")) and g["S"] == 1
    hip.gemm_grouped([a], precision=precision)
    hip.gemm(X["A"], X["B"], ta=bool(ta), tb=bool(tb), bias=X["bias"], epilogue=GC.EPI_BIAS_ELU, out=b["out"], use_workspace=False, precision=precision)
    torch.cuda.synchronize()
    assert_bits(a["out"], b["out"], "lone grouped against the single entry")


# entry, (ta, tb, M, N, K), precision, extra: ragged M and N on every body
REVERSAL_CASES = {
    "gemm_kw4": ("gemm", (0, 0, 37, 50, 70), F32, {}),
    "gemm_kw4_splitk": ("gemm", (0, 1, 21, 27, 1030), BF16, {}),
    "gemm_kw1": ("gemm", (1, 0, 1010, 2050, 20), F32, {}),
    "gemm_kw1_bf16": ("gemm", (0, 0, 1010, 2050, 20), BF16, {}),
    "grouped_long_k": ("grouped", (0, 1, 21, 45, 520), F32, {}),
    "grouped_tile32": ("grouped", (1, 1, 810, 501, 24), BF16, {}),
    "wide_nn": ("grouped", (0, 0, 126, 2064, 20), F32, {}),
    "wide_tn": ("grouped", (1, 0, 520, 516, 256), F32, {}),
    "wide16_nts": ("grouped", (0, 1, 250, 2130, 12), BF16, {}),
    "wide16_nt": ("grouped", (0, 1, 125, 2063, 512), BF16, {}),
    "shortk": ("grouped", (1, 0, 4099, 192, 48), F32, {}),
}


@pytest.mark.parametrize("which", list(REVERSAL_CASES))
def test_rows_and_columns_reversed(hip, which):
    """reversing the rows of op(A) reverses the rows of C, reversing the columns of op(B) its columns: an element's K order does not
    depend on the tile (or slab) it falls into, nor on its place inside it"""
    entry, (ta, tb, M, N, K), prec, _ = REVERSAL_CASES[which]
    gen = torch.Generator().manual_seed(211 + len(which))
    X = _plain(gen, ta, tb, M, N, K)
    rev_a = dict(X, A=X["A"].flip(1 if ta else 0).contiguous())
    rev_b = dict(X, B=X["B"].flip(0 if tb else 1).contiguous())
    runs = [_fresh(X), _fresh(rev_a), _fresh(rev_b)]
    if entry == "grouped":
        assert len({_body(hip, [r], prec) for r in runs}) == 1
    for r in runs:
        if entry == "grouped":
            hip.gemm_grouped([r], precision=prec)
        else:
            hip.gemm(r["A"], r["B"], ta=bool(ta), tb=bool(tb), out=r["out"], precision=prec)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(runs[0]["out"]).all())
    assert_bits(runs[1]["out"].flip(0).contiguous(), runs[0]["out"], which + ": rows of op(A) reversed")
    assert_bits(runs[2]["out"].flip(1).contiguous(), runs[0]["out"], which + ": columns of op(B) reversed")


@pytest.mark.parametrize("name", ["wide16_nn_a1b1", "wide16_nt_a1b1", "wide16_nts_a1b1", "wide16_nn_a1b1_lone", "big_bf16_14", "big_bf16_handover"])
def test_mirror_combinations_agree(hip, name):
    """operands read from their bf16 mirrors against rounded in registers: the four A16 / B16 combinations give the same C and C16"""
    ref = None
    for mirrors in ((False, False), (True, False), (False, True), (True, True)):
        staged = stage(name, mirrors=mirrors)
        launch(hip, name, staged)
        torch.cuda.synchronize()
        outs = [(s["outputs"]["C"][2].clone(), s["outputs"]["C16"][2].clone() if "C16" in s["outputs"] else None) for s in staged]
        if ref is None:
            ref = outs
        for i, ((c, c16), (rc, rc16)) in enumerate(zip(outs, ref)):
            assert_bits(c.contiguous(), rc.contiguous(), f"{name}[{i}] C with mirrors {mirrors}")
            if c16 is not None:
                assert_bits(c16.contiguous(), rc16.contiguous(), f"{name}[{i}] C16 with mirrors {mirrors}")


@pytest.mark.parametrize("name", ["gemm_bf16_nn_epi1", "gemm_bf16_tn_epi2", "gemm_bf16_kw1_nt_epi1", "gemm_bf16_splitk4_epi0", "grouped_bf16_tile16",
                                  "grouped_bf16_long_k", "grouped_c16_tile32", "wide16_nn_a0b0", "wide16_nts_a0b0", "big_bf16_14"])
def test_pre_rounded_operand(hip, name):
    """precision 1 on A against precision 1 on bf16(A) stored as float32: rounding is idempotent, so the same bits"""
    outs = []
    for pre in (False, True):
        staged = stage(name, mirrors=(False, False), pre_round_a=pre)
        launch(hip, name, staged)
        torch.cuda.synchronize()
        outs.append([s["outputs"]["C"][2].clone() for s in staged])
    for i, (a, b) in enumerate(zip(*outs)):
        assert_bits(a.contiguous(), b.contiguous(), f"{name}[{i}] pre-rounded A")
