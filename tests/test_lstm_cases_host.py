"""The cases of tests/test_lstm_kernels.py on the CPU: every case builds (its conditions are asserted where its inputs are made,
tests/lstm_cases.py, and again here), every case lands on the kernel body its table row names when held against the host mirrors of
the dispatch rules (attend_infer_repeat_amd/gemm_groups.py), every (entry, kernel body, precision) behind the LSTM entries is reached
by at least one case, the mirrors agree with the library's exported rule and with a table of edges derived by hand, lstm_bwd64 and
chain64 agree with torch.autograd on the float64 forward, and the plain float32 restatement of every comparison stays within a quarter
of the bound the GPU test holds the kernels to."""
import pytest
import torch

import lstm_cases as LC
from attend_infer_repeat_amd import gemm_groups as G
from lstm_cases import BF16, F32, PLANTED, UNIT

SHARE = LC.RESTATEMENT_SHARE


def _tiles(M, Hd):
    return ((M + 15) // 16) * ((Hd + 15) // 16)


# ---- the references against independent ones --------------------------------------------------------------------------------------
def test_forward_reference_is_lstm64():
    c = LC.fwd_case(37, 50, UNIT, BF16, -2.5)
    for a, b in zip(LC.lstm_fwd_ref(c["h_prev"], c["c_prev"], c["w_h"], c["gx"], -2.5, BF16), (c["h64"], c["c64"], c["act64"])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pattern", sorted(LC.PATTERNS))
def test_lstm_bwd64_against_autograd(pattern):
    """d/d pre, d/d c_prev of sum(h * dh) + sum(c * dc_in) through the float64 step, h's gradient being dgates_next . w_h^T + dh_a + dh_b"""
    M, Hd = 37, 50
    f, b = LC.fwd_case(M, Hd, UNIT, F32, 1.0), LC.bwd_case(M, Hd, UNIT)
    dh_a, dh_b, dc_in, dgx_in = LC.pattern_operands(b, pattern)
    pre = (f["h_prev"].double() @ f["w_h"].double() + f["gx"].double()).requires_grad_(True)
    cp = f["c_prev"].double().requires_grad_(True)
    i, j, fg, o = torch.chunk(pre, 4, -1)
    c = torch.sigmoid(fg + 1.0) * cp + torch.sigmoid(i) * torch.tanh(j)
    h = torch.tanh(c) * torch.sigmoid(o)
    dh = b["dgates_next"].double() @ b["w_h"].double().t()
    for t in (dh_a, dh_b):
        dh = dh + (0 if t is None else t.double())
    L = (h * dh).sum() + (0 if dc_in is None else (c * dc_in.double()).sum())
    gp, gc = torch.autograd.grad(L, [pre, cp])
    # the link evaluated on the float64 activations (the case hands the kernel their float32 values: compared on those below)
    act = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(fg + 1.0), torch.sigmoid(o)], -1).detach()
    d, dcp, dgx = LC.lstm_bwd64(b["dgates_next"], b["w_h"], dh_a, dh_b, dc_in, act, cp.detach(), c.detach(), dgx_in)
    scale = 1 + float(gp.abs().max())
    assert float((d - gp).abs().max()) < 1e-12 * scale and float((dcp - gc).abs().max()) < 1e-12 * scale
    assert torch.equal(dgx, d if dgx_in is None else dgx_in.double() + d)
    # ... and on the float32 saved state of the case: the rounding of gate_act / c moves it by a few float32 ulps only
    d32, dcp32, _ = LC.bwd_ref(M, Hd, UNIT, F32, pattern)
    assert LC.ratio(d32, gp, LC.BWD_TOL) < 0.1 and LC.ratio(dcp32, gc, LC.BWD_TOL) < 0.1


@pytest.mark.parametrize("T", [1, 2, 3, 8])
def test_chain64_against_autograd(T):
    c = LC.chain_case(21, 48, T)
    M, Hd, ref = c["M"], c["Hd"], c["ref"]
    w = c["w_h"].double()
    c0 = c["c0"].double()[None, :].expand(M, -1).clone().requires_grad_(True)
    zs = [torch.zeros(M, 4 * Hd, dtype=torch.float64, requires_grad=True) for _ in range(T)]         # pre_t = h . w + gx + z_t
    h, cc, L = c["h0"].double()[None, :].expand(M, -1), c0, 0.0
    for t in range(T):
        pre = h @ w + c["gx"].double() + zs[t]
        i, j, f, o = torch.chunk(pre, 4, -1)
        cc = torch.sigmoid(f + 1.0) * cc + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(cc) * torch.sigmoid(o)
        L = L + (h * (c["dH"][t].double() + c["dH_b"][t].double())).sum()
        assert float((h.detach() - ref["h_seq"][t + 1]).abs().max()) < 1e-13 and float((cc.detach() - ref["c_seq"][t + 1]).abs().max()) < 1e-12
    grads = torch.autograd.grad(L, zs + [c0])
    scale = 1 + max(float(x.abs().max()) for x in grads)
    for t in range(T):
        assert float((grads[t] - ref["dgates"][t]).abs().max()) < 1e-12 * scale, t
        assert float((sum(grads[t:T]) - ref["dgx_after"][t]).abs().max()) < 1e-12 * scale, t
    assert float((grads[T] - ref["dc0"]).abs().max()) < 1e-12 * scale
    assert torch.equal(ref["dgx_after"][T - 1], ref["dgates"][T - 1])                               # T = 1 leaves dgx = dgates[0]
    assert torch.equal(ref["h_seq"][0], c["h0"].double()[None, :].expand(M, -1))


# ---- the planted regime ------------------------------------------------------------------------------------------------------------
def test_planted_tensors_hold_every_value_and_saturate():
    c = LC.fwd_case(5, 7, PLANTED, F32, 1.0)                     # the smallest case: 35 cell states for 15 values
    for v in LC.GX_LIST:
        assert bool((c["gx"] == v).any())
    for v in LC.C_LIST:
        assert bool((c["c_prev"] == v).any())
    assert max(LC.GX_LIST) == 90 and min(LC.GX_LIST) == -90 and max(LC.C_LIST) == 60 and min(LC.C_LIST) == -60
    # expf(90) overflows float32: sigmoid_acc(-90) is exactly 0, and float32 tanh is exactly +-1 from |x| = 17 / on the plateau of c
    assert float(torch.exp(torch.tensor(90.0))) == float("inf") and float(torch.tanh(torch.tensor(17.0))) == 1.0
    a32 = LC.lstm_fwd_ref(c["h_prev"], c["c_prev"], c["w_h"], c["gx"], 1.0, F32, torch.float32)[2]
    assert bool((a32 == 0).any()) and bool((a32 == 1).any()) and bool((a32 == -1).any())
    assert float(c["act64"][c["act64"] > 0].min()) < 1e-38     # float64 keeps what float32 drops
    b = LC.bwd_case(5, 7, PLANTED)
    Hd = 7
    ifo = torch.cat([b["gate_act"][:, :Hd], b["gate_act"][:, 2 * Hd:]], 1)
    for v in LC.GATE_LIST:
        v32 = torch.tensor(v, dtype=torch.float32)
        assert bool((ifo == v32).any()) and bool((b["gate_act"][:, Hd:2 * Hd] == v32).any())
        assert v == 0 or bool((b["gate_act"][:, Hd:2 * Hd] == -v32).any())                       # gj in both signs
    assert bool((ifo >= 0).all())
    assert float(torch.tensor(LC.GATE_LIST[4], dtype=torch.float32)) == 1.0 - 2.0 ** -24         # representable: one ulp below 1
    e = LC.entry_case(5, 16, PLANTED)
    assert bool((e["c2"].abs() >= 44).any()) and bool((e["c2"].abs() < 44).any())
    with pytest.raises(AssertionError):
        LC.planted(torch.Generator().manual_seed(0), (2, 3), LC.C_LIST)                            # too small to hold its extremes


# ---- every case builds and lands where its row says ---------------------------------------------------------------------------------
def test_forward_runs_build_and_reach_their_body():
    pads, seen = {}, set()
    for (M, Hd, layout, body, pad, regime, fb, precision) in LC.FWD_RUNS:
        assert LC.fwd_body(M, Hd, layout) == body, (M, Hd, layout)
        c = LC.fwd_case(M, Hd, regime, precision, fb)
        assert c["h64"].shape == (M, Hd) and c["act64"].shape == (M, 4 * Hd)
        pads.setdefault((M, Hd, layout), set()).add(pad); seen.add((regime, fb, precision))
    assert all(p == {3, 8} for p in pads.values()) and len(pads) == len(LC.FWD_SHAPES)
    for regime in (UNIT, PLANTED):
        assert {fb for r, fb, _ in seen if r == regime} == set(LC.FORGET_BIASES)
    # the edge: 512 tiles fused, 513 and beyond wide, and the two layouts that keep 528 tiles on the 4-wave kernel
    assert _tiles(512, 256) == _tiles(2048, 64) == 512 and _tiles(513, 256) == 528 and _tiles(2049, 64) == 516
    assert not G.lstm_fwd_wide(8192, 4) and not G.lstm_fwd_wide(8208, 4) and G.lstm_fwd_wide(528, 256)
    assert G.lstm_fwd_wide(513, 256) and not G.lstm_fwd_wide(513, 256, h_prev=4) and not G.lstm_fwd_wide(513, 256, ldw=1027)
    assert not G.lstm_fwd_wide(513, 256, w_h=4) and not G.lstm_fwd_wide(2049, 50)
    bits = [(M, Hd) for M, Hd, layout, *_ in LC.FWD_SHAPES if LC.fwd_pair_is_bitwise(M, Hd, layout)]
    assert bits == [(5, 7), (37, 50), (130, 40), (64, 256)]     # elsewhere the product runs on 32 x 32 tiles or the wide-tile kernels
    for run in LC.PW_FWD_RUNS + LC.PW_BWD_RUNS:
        assert run[0] > 0
    assert 2049 * 256 > 2048 * 256                                # the element loop of the pointwise kernels goes round


def test_backward_runs_build_and_reach_their_body():
    for (M, Hd, layout, body, regime, precision) in LC.BWD_RUNS:
        assert LC.bwd_body(M, Hd, layout) == body, (M, Hd, layout)
        c = LC.bwd_case(M, Hd, regime)
        assert c["gate_act"].shape == (M, 4 * Hd)
    bits = [(M, Hd, layout) for M, Hd, layout, _ in LC.BWD_SHAPES if LC.bwd_pair_is_bitwise(M, Hd, layout)]
    assert bits == [(64, 256, ""), (513, 256, "dgn_off"), (513, 256, "w_off"), (2049, 50, "")]
    # lstm_bwd_launch, derived by hand: 512 / 513 tiles in each direction, and what keeps a launch of more off the wide kernel
    table = [((512, 256), {}, "kw16"), ((513, 256), {}, "wide"), ((8192, 16), {}, "kw16"), ((8193, 16), {}, "kw4"),
             ((16, 8192), {}, "kw16"), ((16, 8208), {}, "kw4"), ((16, 8256), {}, "wide"), ((513, 256), dict(dgates_next=4), "kw4"),
             ((513, 256), dict(w_h=4), "kw4"), ((513, 256), dict(w_h=16), "wide"), ((2049, 50), {}, "kw4"), ((2049, 64), {}, "wide"),
             ((2048, 64), {}, "kw16"), ((1, 1), {}, "kw16")]
    for shape, kw, form in table:
        assert G.lstm_bwd_form(*shape, **kw) == form, (shape, kw)


def test_entry_and_bf16_rules_against_the_table_and_the_library():
    for M, Hd, fits in LC.ENTRY_FITS_TABLE:
        assert G.lstm_bwd_entry_fits(M, Hd) == fits, (M, Hd)
    for M, Hd in LC.ENTRY_SHAPES:
        assert G.lstm_bwd_entry_fits(M, Hd)
    assert _tiles(512, 256) == 512 and not G.lstm_bwd_entry_fits(513, 256) and not G.lstm_bwd_entry_fits(37, 50)
    assert G.lstm_bf16_fits(48, 64) and not G.lstm_bf16_fits(48, 50) and not G.lstm_bf16_fits(0, 64) and not G.lstm_bf16_fits(48, 32)
    try:
        from attend_infer_repeat_amd import _lib
        lib = _lib.load()
    except Exception:                                             # no library on this host: the table above stands alone
        return
    for M in (0, 1, 16, 17, 64, 511, 512, 513, 2048, 2049, 8192, 8193):
        for Hd in (0, 8, 16, 48, 50, 64, 250, 256, 512, 8192, 8208):
            assert bool(lib.air_lstm_step_bwd_entry_fits(M, Hd)) == G.lstm_bwd_entry_fits(M, Hd), (M, Hd)


def test_every_entry_body_and_precision_is_reached():
    got = LC.reached()
    missing = sorted(LC.DECLARED - set(got))
    assert not missing, f"reached by no case: {missing}"
    assert set(got) <= LC.DECLARED, sorted(set(got) - LC.DECLARED)


def test_chain_cases_build():
    for M, Hd, T in LC.CHAIN_RUNS:
        c = LC.chain_case(M, Hd, T)
        assert c["ref"]["dgates"].shape == (T, M, 4 * Hd) and c["ref"]["dc0"].shape == (M, Hd)
    assert {T for _, _, T in LC.CHAIN_RUNS} == {1, 2, 3, 8}
    assert LC.chain_uses_entry(21, 48, 2) and not LC.chain_uses_entry(21, 48, 1) and not LC.chain_uses_entry(2049, 64, 3)
    assert not LC.chain_uses_entry(2049, 50, 2)
    for M, Hd, T, mem16 in LC.CHAIN16_RUNS:
        assert not mem16 or G.lstm_bf16_fits(M, Hd)
    c = LC.rider_case()
    assert all(bool(torch.isfinite(t).all()) for t in c["ref"])


# ---- the float32 restatement of every comparison: within a quarter of the bound the kernels are held to ----------------------------
def test_restatement_forward():
    worst = 0.0
    runs = {(M, Hd, regime, precision, fb) for (M, Hd, _, _, _, regime, fb, precision) in LC.FWD_RUNS}
    runs |= {(M, Hd, regime, BF16, 1.0) for M, Hd, _, regime in LC.BF16MEM_RUNS}
    for (M, Hd, regime, precision, fb) in sorted(runs):
        c = LC.fwd_case(M, Hd, regime, precision, fb)
        got = LC.lstm_fwd_ref(c["h_prev"], c["c_prev"], c["w_h"], c["gx"], fb, precision, torch.float32)
        r = max(LC.ratio(a, c[k], LC.LSTM_TOL) for a, k in zip(got, ("h64", "c64", "act64")))
        assert r <= SHARE, (M, Hd, regime, precision, fb, r)
        worst = max(worst, r)
    for (M, Hd, regime, fb, _) in LC.PW_FWD_RUNS:
        c = LC.fwd_case(M, Hd, regime, F32, fb)
        z = torch.zeros(M, 1), torch.zeros(1, 4 * Hd)
        ref = LC.lstm_fwd_ref(z[0], c["c_prev"], z[1], c["gx"], fb, F32)
        got = LC.lstm_fwd_ref(z[0], c["c_prev"], z[1], c["gx"], fb, F32, torch.float32)
        worst = max(worst, max(LC.ratio(a, b, LC.LSTM_TOL) for a, b in zip(got, ref)))
    assert worst <= SHARE
    print(f"\n[lstm cases] float32 restatement, forward: worst share of the bound {worst:.3g}")


def test_restatement_backward():
    worst = {}
    runs = {(M, Hd, regime, precision) for (M, Hd, _, _, regime, precision) in LC.BWD_RUNS}
    runs |= {(M, Hd, regime, BF16) for M, Hd, _, regime in LC.BF16MEM_RUNS} | {(M, Hd, regime, F32) for M, Hd, regime in LC.PW_BWD_RUNS}
    for (M, Hd, regime, precision) in sorted(runs):
        for pattern in LC.PATTERNS:
            ref = LC.bwd_ref(M, Hd, regime, precision, pattern)
            got = LC.bwd_ref(M, Hd, regime, precision, pattern, torch.float32)
            r = max(LC.ratio(a, b, LC.BWD_TOL) for a, b in zip(got, ref))
            assert r <= SHARE, (M, Hd, regime, precision, pattern, r)
            worst[regime] = max(worst.get(regime, 0.0), r)
    print(f"\n[lstm cases] float32 restatement, one link: worst share of the bound {worst}")


def test_restatement_entry_and_chains():
    worst = 0.0
    for (M, Hd, regime) in LC.ENTRY_RUNS:
        c = LC.entry_case(M, Hd, regime)
        for variant in LC.ENTRY_VARIANTS:
            ref, got = LC.entry_ref(c, variant), LC.entry_ref(c, variant, torch.float32)
            r = max(LC.ratio(a, b, LC.BWD_TOL) for a, b in zip(got, ref) if b is not None)
            assert r <= SHARE, (M, Hd, regime, variant, r)
            worst = max(worst, r)
    print(f"\n[lstm cases] float32 restatement, entry: worst share of the bound {worst:.3g}")
    # the entry's tanh form against tanh, both in float32: what ENTRY_PAIR_TOL_LAST_PLANTED was derived from
    r = {UNIT: [0.0, 0.0], PLANTED: [0.0, 0.0]}
    for (M, Hd, regime) in LC.ENTRY_RUNS:
        for variant in LC.ENTRY_VARIANTS[:3]:
            c = LC.entry_case(M, Hd, regime)
            fast, libm = LC.entry_last32(c, variant, True), LC.entry_last32(c, variant, False)
            r[regime] = [max(w, LC.ratio(a, b, LC.ENTRY_PAIR_TOL_LAST)) for w, a, b in zip(r[regime], fast, libm)]
    print(f"[lstm cases] the entry's tanh form against tanh in float32, share of 1e-6 |ref| + 1e-6 (dgates1, dc_prev1): {r}")
    assert max(r[UNIT]) <= 1.0 and r[PLANTED][1] <= 1.0
    assert 1.0 < r[PLANTED][0] <= LC.ENTRY_FAST_TANH_R * 1.05          # (the host's own exp decides the last digits)
    assert LC.ENTRY_PAIR_TOL_LAST_PLANTED == (8 * LC.ENTRY_FAST_TANH_R * 1e-6,) * 2
    worst = 0.0
    for (M, Hd, T) in LC.CHAIN_RUNS:
        c = LC.chain_case(M, Hd, T)
        got = LC.chain64(c["h0"], c["c0"], c["w_h"], c["gx"], T, c["dH"], c["dH_b"], dtype=torch.float32)
        for k, ref in c["ref"].items():
            r = LC.ratio(got[k], ref, LC.LSTM_TOL if k in ("h_seq", "c_seq", "gate_act") else LC.BWD_TOL)
            assert r <= SHARE, (M, Hd, T, k, r)
            worst = max(worst, r)
    print(f"\n[lstm cases] float32 restatement, chains: worst share of the bound {worst:.3g}")
