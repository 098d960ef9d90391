"""GPU parity of the LSTM recurrence, one launch at a time (run with -m gpu on an MI355X): the forward steps with a full h_prev
(air_lstm_step_fwd, air_lstm_step_fwd_bf16, air_lstm_pointwise_fwd), one BPTT link (air_lstm_step_bwd[_opt], air_lstm_step_bwd_bf16,
air_lstm_pointwise_bwd[_bf16 / _opt]), the entry of the BPTT folded into its first link (air_lstm_step_bwd_entry), chains wired as
engine_plan._PlanBuilder.bptt wires them, and what every entry refuses.

Cases and float64 references come from tests/lstm_cases.py (built and cross-checked on the CPU by tests/test_lstm_cases_host.py, which
also proves that every kernel body behind the entries is reached).  Every input sits in a buffer with two more rows of NaN behind it
(and NaN in the padding columns of a gx / w_h view), every output starts as NaN in a buffer whose two last rows hold a sentinel that
is compared afterwards.  Each fused launch is held twice: against float64 at the bound of the older tests, and against the launches it
replaces -- bit for bit where attend_infer_repeat_amd/gemm_groups.py says that the product alone runs on the body whose K order the
step repeats, at 1e-5 elsewhere (the forward on 32 x 32 tiles / the wide-tile kernels from 1000 tiles of gates on; the link on 16
waves where the product alone is no long-K problem, and on its wide kernel).

Group letters (L forward, M one link, N entry, O chains, P refusals, Q optimiser riders) tag every comparison; the worst error /
tolerance ratio of each group is printed when the module finishes (pytest -s)."""
import ctypes

import pytest
import torch

import lstm_cases as LC
from lstm_cases import BF16, BWD_TOL, F32, LSTM_TOL, PAIR_TOL, PLANTED, SENTINEL, UNIT, assert_bits, assert_close, print_worst

pytestmark = pytest.mark.gpu
NAN = float("nan")
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -5


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    LC.WORST.setdefault("P", (0.0, "status codes and untouched bits only"))
    print_worst("lstm kernels", "LMNOPQ")


def dev(t, off=0, ld=None):
    """t[M, n] on the device as a view of a buffer of M + 2 rows of leading dimension ld (default n), everything else in it NaN; off = 1:
    the view starts 4 bytes past a 16-byte boundary"""
    if t is None:
        return None
    M, n = t.shape
    ld = n if ld is None else ld
    flat = torch.full(((M + 2) * ld + 4,), NAN, dtype=torch.float32, device="cuda")
    v = flat[off:off + (M + 2) * ld].view(M + 2, ld)[:M, :n]
    v.copy_(t.cuda())
    assert v.data_ptr() % 16 == 4 * off
    return v


def out(M, n, init=None):
    """-> (buffer [M + 2, n], its first M rows): NaN (or `init`) where the launch writes, the sentinel in the two rows behind"""
    buf = torch.full((M + 2, n), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:M] = NAN if init is None else init.cuda()
    return buf, buf[:M]


def out16(M, n):
    buf = torch.full((M + 2, n), 7.0, dtype=torch.bfloat16, device="cuda")
    buf[:M] = NAN
    return buf, buf[:M]


def tails(bufs, M, what):
    for i, b in enumerate(bufs):
        if b is not None:
            tail = b[M:]
            assert bool((tail == (7.0 if tail.dtype == torch.bfloat16 else SENTINEL)).all()), f"{what}: output {i} written past row M"


def mirror_is_bf16_of(m16, x, what):
    assert torch.equal(m16.view(torch.int16), x.to(torch.bfloat16).view(torch.int16)), what + ": the bf16 mirror is not bf16 of the float32 value"


def pair(a, b, bitwise, what, group):
    if bitwise:
        assert_bits(a, b, what + " against the unfused pair")
    else:
        assert_close(a, b, *PAIR_TOL, what + " against the unfused pair", group)


# ---------------------------------------------------------------------------------------------------------------
# L. forward steps with a full h_prev
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", LC.FWD_RUNS, ids=lambda r: "-".join(str(x) for x in r))
def test_lstm_step_fwd(hip, run):
    """air_lstm_step_fwd against float64 and against product + air_lstm_pointwise_fwd.  The older test's docstring said "bitwise" of
    the pair and asserted 1e-5.  Bits are asserted where the product alone runs on the 4-wave 16 x 16 body (LC.fwd_pair_is_bitwise:
    the sum over K, the wave reduction and + gx are the same sums in the same order); elsewhere the product's K order is another one
    and 1e-5 stays.  When this test was written gate_act held bit for bit there and c, h did not (5798 of 16 384 elements of c at
    64 x 256): the fused kernels round the cell update as fma(gf, c_prev, gi * gj), lstm_pw_fwd_kernel had fma(gi, gj, gf * c_prev).
    The pointwise kernel now writes the first form out."""
    M, Hd, layout, body, pad, regime, fb, precision = run
    c = LC.fwd_case(M, Hd, regime, precision, fb)
    tag = f"step_fwd {run} "
    h_prev, c_prev = dev(c["h_prev"], off=1 if layout == "h_off" else 0), dev(c["c_prev"])
    w_h = dev(c["w_h"], ld=4 * Hd + 3 if layout == "ldw3" else None)
    gx = dev(c["gx"], ld=4 * Hd + pad)
    bufs, views = zip(out(M, Hd), out(M, Hd), out(M, 4 * Hd))
    h, cc, act = hip.lstm_step_fwd(h_prev, c_prev, w_h, gx, fb, precision, out=views)
    gates = hip.gemm_grouped([dict(A=h_prev, B=w_h, epilogue=hip.EPI_ADD_AUX, aux=gx)], precision=precision)[0][0]
    hu, cu, actu = hip.lstm_pointwise_fwd(gates, c_prev, fb)
    torch.cuda.synchronize()
    assert_close(h, c["h64"], *LSTM_TOL, tag + "h", "L"); assert_close(cc, c["c64"], *LSTM_TOL, tag + "c", "L")
    assert_close(act, c["act64"], *LSTM_TOL, tag + "gate_act", "L")
    tails(bufs, M, tag)
    bitwise = LC.fwd_pair_is_bitwise(M, Hd, layout)
    pair(act, actu, bitwise, tag + "gate_act", "L"); pair(cc, cu, bitwise, tag + "c", "L"); pair(h, hu, bitwise, tag + "h", "L")


@pytest.mark.parametrize("run", LC.PW_FWD_RUNS, ids=str)
def test_lstm_pointwise_fwd(hip, run):
    M, Hd, regime, fb, with_act = run
    c = LC.fwd_case(M, Hd, regime, F32, fb)
    tag = f"pointwise_fwd {run} "
    zm, zw = torch.zeros(M, 1), torch.zeros(1, 4 * Hd)
    h64, c64, act64 = LC.lstm_fwd_ref(zm, c["c_prev"], zw, c["gx"], fb, F32)
    bufs, views = zip(out(M, Hd), out(M, Hd), out(M, 4 * Hd))
    h, cc, act = hip.lstm_pointwise_fwd(dev(c["gx"]), dev(c["c_prev"]), fb, out=views if with_act else views[:2] + (None,), want_act=with_act)
    torch.cuda.synchronize()
    assert_close(h, h64, *LSTM_TOL, tag + "h", "L"); assert_close(cc, c64, *LSTM_TOL, tag + "c", "L")
    if with_act:
        assert_close(act, act64, *LSTM_TOL, tag + "gate_act", "L")
    else:
        assert act is None and bool(torch.isnan(views[2]).all()), tag + "gate_act = NULL: nothing written"
    tails(bufs, M, tag)


@pytest.mark.parametrize("run", LC.BF16MEM_RUNS, ids=str)
def test_lstm_step_fwd_bf16(hip, run):
    M, Hd, mirrors, regime = run
    c = LC.fwd_case(M, Hd, regime, BF16, 1.0)
    tag = f"step_fwd_bf16 {run} "
    h_prev, c_prev, gx = dev(c["h_prev"]), dev(c["c_prev"]), dev(c["gx"], ld=4 * Hd + 8)
    w16 = c["w_h"].cuda().to(torch.bfloat16)
    bufs, views = zip(out(M, Hd), out(M, Hd), out(M, 4 * Hd))
    b16, h16 = out16(M, Hd)
    h, cc, act = hip.lstm_step_fwd_bf16(h_prev, c_prev, w16, gx, 1.0, h_prev_bf16=h_prev.to(torch.bfloat16) if mirrors else None, h_bf16=h16,
                                        out=views)
    torch.cuda.synchronize()
    assert_close(h, c["h64"], *LSTM_TOL, tag + "h", "L"); assert_close(cc, c["c64"], *LSTM_TOL, tag + "c", "L")
    assert_close(act, c["act64"], *LSTM_TOL, tag + "gate_act", "L")
    mirror_is_bf16_of(h16, h, tag + "h")
    tails(bufs + (b16,), M, tag)
    # without the output mirror: the same float32 bits
    bufs2, views2 = zip(out(M, Hd), out(M, Hd), out(M, 4 * Hd))
    hip.lstm_step_fwd_bf16(h_prev, c_prev, w16, gx, 1.0, h_prev_bf16=h_prev.to(torch.bfloat16) if mirrors else None, out=views2)
    torch.cuda.synchronize()
    for a, b in zip(views, views2):
        assert_bits(a, b, tag + "with and without h_bf16")


# ---------------------------------------------------------------------------------------------------------------
# M. one BPTT link
# ---------------------------------------------------------------------------------------------------------------
def _link_operands(c, pattern, dgn, M, Hd):
    """device operands of a pattern and the dgx buffer: -> dh_a, dh_b, dc_in, dgx_in, (dgx buffer, view) | (None, None)"""
    dh_a, dh_b, dc_in, _ = (dev(t) for t in LC.pattern_operands(c, pattern))
    kind, want = LC.PATTERNS[pattern][3], LC.PATTERNS[pattern][4]
    bx, vx = out(M, 4 * Hd, c["dgx_in"] if kind == "inplace" else None) if want else (None, None)
    dgx_in = {None: None, "own": dev(c["dgx_in"]), "inplace": vx, "next": dgn}[kind]
    return dh_a, dh_b, dc_in, dgx_in, bx, vx


@pytest.mark.parametrize("run", LC.BWD_RUNS, ids=lambda r: "-".join(str(x) for x in r))
def test_lstm_step_bwd(hip, run):
    M, Hd, layout, body, regime, precision = run
    c = LC.bwd_case(M, Hd, regime)
    dgn, w_h = dev(c["dgates_next"], off=1 if layout == "dgn_off" else 0), dev(c["w_h"], off=1 if layout == "w_off" else 0)
    act, c_prev, cc = dev(c["gate_act"]), dev(c["c_prev"]), dev(c["c"])
    bitwise = LC.bwd_pair_is_bitwise(M, Hd, layout)
    for pattern in LC.PATTERNS:
        tag = f"step_bwd {run} {pattern} "
        dh_a, dh_b, dc_in, dgx_in, bx, vx = _link_operands(c, pattern, dgn, M, Hd)
        (bd, vd), (bc, vc) = out(M, 4 * Hd), out(M, Hd)
        dg, dcp, dgx = hip.lstm_step_bwd(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc, dgx_in=dgx_in, precision=precision, out=(vd, vc, vx))
        torch.cuda.synchronize()
        r_dg, r_dcp, r_dgx = LC.bwd_ref(M, Hd, regime, precision, pattern)
        assert_close(dg, r_dg, *BWD_TOL, tag + "dgates", "M"); assert_close(dcp, r_dcp, *BWD_TOL, tag + "dc_prev", "M")
        if vx is not None:
            assert_close(dgx, r_dgx, *BWD_TOL, tag + "dgx", "M")
        else:
            assert dgx is None
        tails((bd, bc, bx), M, tag)
        assert_bits(dgn, c["dgates_next"], tag + "dgates_next left as it was")
        if pattern in ("all", "none"):
            # the launches it replaces: the product accumulating onto dh_a (beta = 1), then the pointwise backward with dh_b as dh2
            base = dh_a.clone() if dh_a is not None else None
            dh = hip.gemm_grouped([dict(A=dgn, B=w_h, tb=True, **(dict(beta=1.0, out=base) if base is not None else {}))], precision=precision)[0][0]
            dgu, dcpu = hip.lstm_pointwise_bwd(act, c_prev, cc, dh, dc_in, dh2=dh_b)
            torch.cuda.synchronize()
            pair(dg, dgu, bitwise, tag + "dgates", "M"); pair(dcp, dcpu, bitwise, tag + "dc_prev", "M")
            if vx is not None:
                pair(dgx, c["dgx_in"].cuda() + dgu, bitwise, tag + "dgx", "M")


@pytest.mark.parametrize("run", LC.BF16MEM_RUNS, ids=str)
def test_lstm_step_bwd_bf16_and_pointwise_bwd_bf16(hip, run):
    M, Hd, mirrors, regime = run
    c = LC.bwd_case(M, Hd, regime)
    dgn, act, c_prev, cc = dev(c["dgates_next"]), dev(c["gate_act"]), dev(c["c_prev"]), dev(c["c"])
    w16 = c["w_h"].cuda().to(torch.bfloat16)
    dgn16 = dgn.to(torch.bfloat16) if mirrors else None
    for pattern in LC.PATTERNS:
        tag = f"step_bwd_bf16 {run} {pattern} "
        dh_a, dh_b, dc_in, dgx_in, bx, vx = _link_operands(c, pattern, dgn, M, Hd)
        (bd, vd), (bc, vc), (bd16, vd16) = out(M, 4 * Hd), out(M, Hd), out16(M, 4 * Hd)
        bx16, vx16 = out16(M, 4 * Hd) if vx is not None else (None, None)
        dg, dcp, dgx = hip.lstm_step_bwd_bf16(dgn, w16, dh_a, dh_b, dc_in, act, c_prev, cc, dgx_in=dgx_in, dgates_next_bf16=dgn16,
                                              dgates_bf16=vd16, dgx_bf16=vx16, out=(vd, vc, vx))
        torch.cuda.synchronize()
        r_dg, r_dcp, r_dgx = LC.bwd_ref(M, Hd, regime, BF16, pattern)
        assert_close(dg, r_dg, *BWD_TOL, tag + "dgates", "M"); assert_close(dcp, r_dcp, *BWD_TOL, tag + "dc_prev", "M")
        mirror_is_bf16_of(vd16, dg, tag + "dgates")
        if vx is not None:
            assert_close(dgx, r_dgx, *BWD_TOL, tag + "dgx", "M"); mirror_is_bf16_of(vx16, dgx, tag + "dgx")
        tails((bd, bc, bx, bd16, bx16), M, tag)
    # the pointwise backward of the last step with its mirror: float64, and the bits of air_lstm_pointwise_bwd
    tag = f"pointwise_bwd_bf16 {run} "
    dh_a, dh_b = dev(c["dh_a"]), dev(c["dh_b"])
    (bd, vd), (bc, vc), (bd16, vd16) = out(M, 4 * Hd), out(M, Hd), out16(M, 4 * Hd)
    dg, dcp = hip.lstm_pointwise_bwd_bf16(act, c_prev, cc, dh_a, None, vd16, dh2=dh_b, out=(vd, vc))
    dg2, dcp2 = hip.lstm_pointwise_bwd(act, c_prev, cc, dh_a, None, dh2=dh_b)
    torch.cuda.synchronize()
    r_dg, r_dcp, _ = LC.lstm_bwd64(None, None, c["dh_a"], c["dh_b"], None, c["gate_act"], c["c_prev"], c["c"])
    assert_close(dg, r_dg, *BWD_TOL, tag + "dgates", "M"); assert_close(dcp, r_dcp, *BWD_TOL, tag + "dc_prev", "M")
    mirror_is_bf16_of(vd16, dg, tag + "dgates"); tails((bd, bc, bd16), M, tag)
    assert_bits(dg, dg2, tag + "dgates against air_lstm_pointwise_bwd"); assert_bits(dcp, dcp2, tag + "dc_prev against air_lstm_pointwise_bwd")


@pytest.mark.parametrize("run", LC.PW_BWD_RUNS, ids=str)
def test_lstm_pointwise_bwd_with_dh2(hip, run):
    M, Hd, regime = run
    c = LC.bwd_case(M, Hd, regime)
    act, c_prev, cc = dev(c["gate_act"]), dev(c["c_prev"]), dev(c["c"])
    for name, (a, b, dc) in {"dh, dh2, dc": ("dh_a", "dh_b", "dc_in"), "dh, dh2": ("dh_a", "dh_b", None), "dh2, dc": (None, "dh_b", "dc_in"),
                             "dc alone": (None, None, "dc_in"), "dh alone": ("dh_a", None, None)}.items():
        tag = f"pointwise_bwd {run} {name} "
        t = lambda k: c[k] if k else None
        (bd, vd), (bc, vc) = out(M, 4 * Hd), out(M, Hd)
        dg, dcp = hip.lstm_pointwise_bwd(act, c_prev, cc, dev(t(a)), dev(t(dc)), dh2=dev(t(b)), out=(vd, vc))
        torch.cuda.synchronize()
        r_dg, r_dcp, _ = LC.lstm_bwd64(None, None, t(a), t(b), t(dc), c["gate_act"], c["c_prev"], c["c"])
        assert_close(dg, r_dg, *BWD_TOL, tag + "dgates", "M"); assert_close(dcp, r_dcp, *BWD_TOL, tag + "dc_prev", "M")
        tails((bd, bc), M, tag)


# ---------------------------------------------------------------------------------------------------------------
# N. air_lstm_step_bwd_entry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", LC.ENTRY_RUNS, ids=str)
def test_lstm_step_bwd_entry(hip, run):
    M, Hd, regime = run
    c = LC.entry_case(M, Hd, regime)
    d = {k: dev(c[k]) for k in ("act1", "act0", "c0", "c1", "c2", "dh_a1", "dh_b1", "dh_a0", "dh_b0", "w_h")}
    for variant in LC.ENTRY_VARIANTS:
        tag = f"bwd_entry {run} {variant} "
        a1 = None if variant == "no dh_a1" else d["dh_a1"]
        b1 = None if variant == "no dh_b1" else d["dh_b1"]
        pairs = [out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd) if variant != "no dgx_out" else (None, None)]
        bufs, views = zip(*pairs)
        dg1, dcp1, dg0, dcp0, dgx = hip.lstm_step_bwd_entry(d["act1"], d["c1"], d["c2"], a1, b1, d["w_h"], d["dh_a0"], d["dh_b0"], d["act0"],
                                                            d["c0"], d["c1"], out=views)
        # the two launches
        dg1u, dcp1u = hip.lstm_pointwise_bwd(d["act1"], d["c1"], d["c2"], a1 if a1 is not None else b1, None, dh2=b1 if a1 is not None else None)
        dg0u, dcp0u, dgxu = hip.lstm_step_bwd(dg1u, d["w_h"], d["dh_a0"], d["dh_b0"], dcp1u, d["act0"], d["c0"], d["c1"], dgx_in=dg1u, want_dgx=True)
        torch.cuda.synchronize()
        tails(bufs, M, tag)
        r = LC.entry_ref(c, variant)
        for got, ref, nm in zip((dg1, dcp1, dg0, dcp0, dgx), r, ("dgates1", "dc_prev1", "dgates", "dc_prev", "dgx")):
            if ref is None:
                assert got is None
            else:
                assert_close(got, ref, *BWD_TOL, tag + nm + " against float64", "N")
        assert_close(dg1, dg1u, *(LC.ENTRY_PAIR_TOL_LAST_PLANTED if regime == PLANTED else LC.ENTRY_PAIR_TOL_LAST),
                     tag + "dgates1 against the two launches", "N")
        assert_close(dcp1, dcp1u, *LC.ENTRY_PAIR_TOL_LAST, tag + "dc_prev1 against the two launches", "N")
        assert_close(dg0, dg0u, *LC.ENTRY_PAIR_TOL_LINK, tag + "dgates against the two launches", "N")
        assert_close(dcp0, dcp0u, *LC.ENTRY_PAIR_TOL_LINK, tag + "dc_prev against the two launches", "N")
        if dgx is not None:
            assert_close(dgx, dgxu, *LC.ENTRY_PAIR_TOL_LINK, tag + "dgx against the two launches", "N")
        if regime == PLANTED:
            # on the plateau the fast tanh reaches its limits exactly: 1 - tc * tc is 0, nothing flows into the cell
            flat = (c["c2"].abs() >= 44).cuda()
            assert bool(flat.any())
            for q in range(3):
                assert bool((dg1[:, q * Hd:(q + 1) * Hd][flat] == 0).all()), tag + f"dgates1 gate {q} on the plateau"
            assert bool((dcp1[flat] == 0).all()), tag + "dc_prev1 on the plateau"


def test_lstm_step_bwd_entry_fits(hip):
    lib = hip.lib()
    for M, Hd, fits in LC.ENTRY_FITS_TABLE:
        assert bool(lib.air_lstm_step_bwd_entry_fits(M, Hd)) == fits, (M, Hd)


# ---------------------------------------------------------------------------------------------------------------
# O. chains wired as _PlanBuilder.bptt wires them
# ---------------------------------------------------------------------------------------------------------------
def _run_chain(hip, c, precision, mem16, stepwise, tag):
    """forward T steps, then the backward with the engine's wiring: alternating dc buffers, the running dgx in place, dgates[T-1] as the
    first running sum, the entry fold where the engine folds it (float32, T >= 2, fits).  stepwise: every launch is compared with its
    float64 reference evaluated on what the launches before it wrote (group O).  -> dict of the device results"""
    M, Hd, T = c["M"], c["Hd"], c["T"]
    w_h, gx = dev(c["w_h"]), dev(c["gx"], ld=4 * Hd + 8)
    w16 = c["w_h"].cuda().to(torch.bfloat16) if mem16 else None
    dH, dH_b = [dev(c["dH"][t]) for t in range(T)], [dev(c["dH_b"][t]) for t in range(T)]
    hs, cs = [dev(c["h0"][None, :].expand(M, -1).contiguous())], [dev(c["c0"][None, :].expand(M, -1).contiguous())]
    acts, h16, bufs, bufs16 = [], [None], [], []
    for t in range(T):
        (bh, vh), (bc, vc), (ba, va) = out(M, Hd), out(M, Hd), out(M, 4 * Hd)
        bufs += [bh, bc, ba]
        if mem16:
            b16, v16 = out16(M, Hd); bufs16.append(b16); h16.append(v16)
            hip.lstm_step_fwd_bf16(hs[t], cs[t], w16, gx, 1.0, h_prev_bf16=h16[t], h_bf16=v16, out=(vh, vc, va))
        else:
            hip.lstm_step_fwd(hs[t], cs[t], w_h, gx, 1.0, precision, out=(vh, vc, va))
        if stepwise:
            torch.cuda.synchronize()
            r = LC.lstm64(hs[t].cpu(), cs[t].cpu(), c["w_h"], c["gx"], 1.0, BF16 if (mem16 or precision) else F32)
            for got, ref, nm in zip((vh, vc, va), r, ("h", "c", "gate_act")):
                assert_close(got, ref, *LSTM_TOL, tag + f"{nm}[{t}] on the state step {t - 1} wrote", "O")
            if mem16:
                mirror_is_bf16_of(v16, vh, tag + f"h[{t}]")
        hs.append(vh); cs.append(vc); acts.append(va)
    dg = [out(M, 4 * Hd) for _ in range(T)]
    dg16 = [out16(M, 4 * Hd) for _ in range(T)] if mem16 else None
    (bdgx, dgx) = out(M, 4 * Hd) if T > 1 else dg[0]
    bx16, dgx16 = out16(M, 4 * Hd) if mem16 else (None, None)
    (bca, dc_a), (bcb, dc_b) = out(M, Hd), out(M, Hd)
    entry = (not mem16) and precision == F32 and LC.chain_uses_entry(M, Hd, T)
    assert entry == (not mem16 and precision == F32 and T >= 2 and hip.lib().air_lstm_step_bwd_entry_fits(M, Hd) == 1)
    dc_in, dc_out, entry_dc = None, dc_a, None
    for t in reversed(range(T)):
        saved = (acts[t], cs[t], cs[t + 1])
        acc = dg[T - 1][1] if t == T - 2 else dgx
        snap = None
        if stepwise and t < T - 1:
            torch.cuda.synchronize()
            snap = (acc.cpu().clone(), dc_in.cpu().clone())
        if entry and t == T - 1:
            entry_dc = dc_out
        elif entry and t == T - 2:
            hip.lstm_step_bwd_entry(acts[T - 1], cs[T - 1], cs[T], dH[T - 1], dH_b[T - 1], w_h, dH[t], dH_b[t], *saved,
                                    out=(dg[T - 1][1], entry_dc, dg[t][1], dc_out, dgx))
        elif mem16 and t == T - 1:
            hip.lstm_pointwise_bwd_bf16(*saved, dH[t], None, dg16[t][1], dh2=dH_b[t], out=(dg[t][1], dc_out))
        elif mem16:
            hip.lstm_step_bwd_bf16(dg[t + 1][1], w16, dH[t], dH_b[t], dc_in, *saved, dgx_in=acc, dgates_next_bf16=dg16[t + 1][1],
                                   dgates_bf16=dg16[t][1], dgx_bf16=dgx16, out=(dg[t][1], dc_out, dgx))
        elif t == T - 1:
            hip.lstm_pointwise_bwd(*saved, dH[t], None, dh2=dH_b[t], out=(dg[t][1], dc_out))
        else:
            hip.lstm_step_bwd(dg[t + 1][1], w_h, dH[t], dH_b[t], dc_in, *saved, dgx_in=acc, precision=precision, out=(dg[t][1], dc_out, dgx))
        if stepwise and not (entry and t >= T - 2):
            torch.cuda.synchronize()
            last = t == T - 1
            r = LC.lstm_bwd64(None if last else dg[t + 1][1].cpu(), None if last else c["w_h"], c["dH"][t], c["dH_b"][t], None if last else snap[1],
                              acts[t].cpu(), cs[t].cpu(), cs[t + 1].cpu(), None if last else snap[0], BF16 if (mem16 or precision) else F32)
            assert_close(dg[t][1], r[0], *BWD_TOL, tag + f"dgates[{t}] on what the launches before wrote", "O")
            assert_close(dc_out, r[1], *BWD_TOL, tag + f"dc_prev[{t}] on what the launches before wrote", "O")
            if not last:
                assert_close(dgx, r[2], *BWD_TOL, tag + f"dgx after step {t} on what the launches before wrote", "O")
                if mem16:
                    mirror_is_bf16_of(dgx16, dgx, tag + f"dgx after step {t}")
            if mem16:
                mirror_is_bf16_of(dg16[t][1], dg[t][1], tag + f"dgates[{t}]")
        dc_in, dc_out = dc_out, (dc_b if dc_out is dc_a else dc_a)
    torch.cuda.synchronize()
    tails(bufs + bufs16 + [b for b, _ in dg] + [bdgx if T > 1 else None, bca, bcb, bx16] + ([b for b, _ in dg16] if mem16 else []), M, tag)
    return dict(h_seq=hs, c_seq=cs, gate_act=acts, dgates=[v for _, v in dg], dgx=dgx, dc0=dc_in, entry=entry)


@pytest.mark.parametrize("run", LC.CHAIN_RUNS, ids=str)
def test_lstm_chain_free_running(hip, run):
    M, Hd, T = run
    c = LC.chain_case(M, Hd, T)
    tag = f"chain {run} "
    got, ref = _run_chain(hip, c, F32, False, False, tag), c["ref"]
    assert got["entry"] == LC.chain_uses_entry(M, Hd, T)
    for t in range(T):
        assert_close(got["h_seq"][t + 1], ref["h_seq"][t + 1], *LSTM_TOL, tag + f"h[{t}]", "O")
        assert_close(got["c_seq"][t + 1], ref["c_seq"][t + 1], *LSTM_TOL, tag + f"c[{t}]", "O")
        assert_close(got["gate_act"][t], ref["gate_act"][t], *LSTM_TOL, tag + f"gate_act[{t}]", "O")
        assert_close(got["dgates"][t], ref["dgates"][t], *BWD_TOL, tag + f"dgates[{t}]", "O")
    assert_close(got["dgx"], ref["dgx_after"][0], *BWD_TOL, tag + "dgx", "O")
    assert_close(got["dc0"], ref["dc0"], *BWD_TOL, tag + "dc0", "O")
    if T == 1:
        assert got["dgx"].data_ptr() == got["dgates"][0].data_ptr()                     # T = 1 leaves dgx = dgates[0]


@pytest.mark.parametrize("run", LC.CHAIN16_RUNS, ids=str)
def test_lstm_chain_bf16_step_by_step(hip, run):
    """precision = 1 and the _bf16 entries: a bf16 rounding boundary may fall differently for a float32 and a float64 h, so every launch
    is held against float64 on the values the launches before it wrote, not against a free-running reference"""
    M, Hd, T, mem16 = run
    _run_chain(hip, LC.chain_case(M, Hd, T), BF16, mem16, True, f"chain16 {run} ")


# ---------------------------------------------------------------------------------------------------------------
# P. refusals: the code, and every output buffer still NaN
# ---------------------------------------------------------------------------------------------------------------
RM, RH = 16, 64


def _refusal_specs():
    """entry -> (arguments of a valid call, indices of its outputs, [(what, {argument index: value}, code)]).  "off" as a value: the
    argument's address plus 4 bytes.  Nothing is launched by a refused call, so a shape beyond the buffers is safe to name."""
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    o = lambda *s: torch.full(s, NAN, dtype=torch.float32, device="cuda")
    b = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    o16 = lambda *s: torch.full(s, NAN, dtype=torch.bfloat16, device="cuda")
    M, H = RM, RH
    null = lambda idx: [(f"argument {i} NULL", {i: None}, E_NULL) for i in idx]
    S = {}
    S["air_lstm_step_fwd"] = ([f(M, H), f(M, H), f(H, 4 * H), 4 * H, f(M, 4 * H), 4 * H, o(M, H), o(M, H), o(M, 4 * H), M, H, 1.0, 0, None], (6, 7, 8),
                              null((0, 1, 2, 4, 6, 7, 8)) + [("M = 0", {9: 0}, E_SHAPE), ("ldw < 4 Hd", {3: 4 * H - 1}, E_SHAPE),
                                                            ("ldgx < 4 Hd", {5: 4 * H - 1}, E_SHAPE), ("precision = 2", {12: 2}, E_UNSUPPORTED)])
    S["air_lstm_step_fwd_bf16"] = ([f(M, H), b(M, H), f(M, H), b(H, 4 * H), 4 * H, f(M, 4 * H), 4 * H, o(M, H), o16(M, H), o(M, H), o(M, 4 * H), M, H, 1.0,
                                    None], (7, 8, 9, 10),
                                   null((0, 2, 3, 5, 7, 9, 10)) + [("M = 0", {11: 0}, E_SHAPE), ("ldw < 4 Hd", {4: 4 * H - 4}, E_SHAPE),
                                                                   ("Hd % 64 != 0", {12: 48}, E_SHAPE), ("h_prev 4 bytes off", {0: "off"}, E_ALIGN),
                                                                   ("w_h_bf16 4 bytes off", {3: "off"}, E_ALIGN),
                                                                   ("h_prev_bf16 4 bytes off", {1: "off"}, E_ALIGN)])
    S["air_lstm_pointwise_fwd"] = ([f(M, 4 * H), f(M, H), o(M, H), o(M, H), o(M, 4 * H), M, H, 1.0, None], (2, 3, 4),
                                   null((0, 1, 2, 3)) + [("M = 0", {5: 0}, E_SHAPE), ("Hd = 0", {6: 0}, E_SHAPE)])
    link = [f(M, 4 * H), f(H, 4 * H), f(M, H), f(M, H), f(M, H), f(M, 4 * H), f(M, H), f(M, H), f(M, 4 * H), o(M, 4 * H), o(M, H), o(M, 4 * H), M, H, 0]
    link_cases = null((0, 1, 5, 6, 7, 9, 10)) + [("M = 0", {12: 0}, E_SHAPE), ("Hd = 0", {13: 0}, E_SHAPE), ("precision = 2", {14: 2}, E_UNSUPPORTED)]
    S["air_lstm_step_bwd"] = (link + [None], (9, 10, 11), link_cases)
    S["air_lstm_step_bwd_opt"] = (link + [None, None], (9, 10, 11), link_cases)
    S["air_lstm_step_bwd_bf16"] = ([f(M, 4 * H), b(M, 4 * H), b(H, 4 * H), f(M, H), f(M, H), f(M, H), f(M, 4 * H), f(M, H), f(M, H), f(M, 4 * H), o(M, 4 * H),
                                    o16(M, 4 * H), o(M, H), o(M, 4 * H), o16(M, 4 * H), M, H, None], (10, 11, 12, 13, 14),
                                   null((0, 2, 6, 7, 8, 10, 12)) + [("M = 0", {15: 0}, E_SHAPE), ("Hd % 64 != 0", {16: 48}, E_SHAPE),
                                                                    ("dgates_next 4 bytes off", {0: "off"}, E_ALIGN),
                                                                    ("w_h_bf16 4 bytes off", {2: "off"}, E_ALIGN),
                                                                    ("dgates_next_bf16 4 bytes off", {1: "off"}, E_ALIGN)])
    pw = [f(M, 4 * H), f(M, H), f(M, H), f(M, H), f(M, H), f(M, H), o(M, 4 * H), o(M, H), M, H]
    pw_cases = null((0, 1, 2, 6, 7)) + [("dh and dc both NULL", {3: None, 5: None}, E_NULL), ("M = 0", {8: 0}, E_SHAPE), ("Hd = 0", {9: 0}, E_SHAPE)]
    S["air_lstm_pointwise_bwd"] = (pw + [None], (6, 7), pw_cases)
    S["air_lstm_pointwise_bwd_opt"] = (pw + [None, None], (6, 7), pw_cases)
    S["air_lstm_pointwise_bwd_bf16"] = ([f(M, 4 * H), f(M, H), f(M, H), f(M, H), f(M, H), f(M, H), o(M, 4 * H), o16(M, 4 * H), o(M, H), M, H, None], (6, 7, 8),
                                        null((0, 1, 2, 6, 7, 8)) + [("dh and dc both NULL", {3: None, 5: None}, E_NULL), ("M = 0", {9: 0}, E_SHAPE)])
    S["air_lstm_step_bwd_entry"] = ([f(M, 4 * H), f(M, H), f(M, H), f(M, H), f(M, H), o(M, 4 * H), o(M, H), f(H, 4 * H), f(M, H), f(M, H), f(M, 4 * H), f(M, H),
                                     f(M, H), o(M, 4 * H), o(M, H), o(M, 4 * H), M, H, None, None], (5, 6, 13, 14, 15),
                                    null((0, 1, 2, 5, 6, 7, 10, 11, 12, 13, 14)) + [
                                        ("dh_a1 and dh_b1 both NULL", {3: None, 4: None}, E_NULL), ("M = 0", {16: 0}, E_UNSUPPORTED),
                                        ("Hd % 16 != 0", {17: 40}, E_UNSUPPORTED), ("513 tiles", {16: 2049}, E_UNSUPPORTED),
                                        ("gate_act1 4 bytes off", {0: "off"}, E_ALIGN), ("c1 4 bytes off", {2: "off"}, E_ALIGN),
                                        ("w_h 4 bytes off", {7: "off"}, E_ALIGN), ("dh_b1 4 bytes off", {4: "off"}, E_ALIGN),
                                        ("dgates1 4 bytes off", {5: "off"}, E_ALIGN)])
    return S


REFUSAL_ENTRIES = ["air_lstm_step_fwd", "air_lstm_step_fwd_bf16", "air_lstm_pointwise_fwd", "air_lstm_step_bwd", "air_lstm_step_bwd_opt",
                   "air_lstm_step_bwd_bf16", "air_lstm_pointwise_bwd", "air_lstm_pointwise_bwd_opt", "air_lstm_pointwise_bwd_bf16",
                   "air_lstm_step_bwd_entry"]


@pytest.mark.parametrize("entry", REFUSAL_ENTRIES)
def test_lstm_entries_refuse_and_write_nothing(hip, entry):
    args, outputs, cases = _refusal_specs()[entry]
    fn = getattr(hip.lib(), entry)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(a, change):
        if torch.is_tensor(a):
            return ctypes.c_void_p(a.data_ptr() + (4 if change == "off" else 0))
        return a
    for what, change, code in cases:
        call = [None if (i in change and change[i] is None) else (change[i] if (i in change and change[i] != "off") else raw(a, change.get(i)))
                for i, a in enumerate(args)]
        call[-1] = stream
        assert fn(*call) == code, f"{entry}: {what}"
        torch.cuda.synchronize()
        for i in outputs:
            assert bool(torch.isnan(args[i]).all()), f"{entry}: {what}: output {i} written"
    # ... and the unchanged call is taken and fills every output
    call = [raw(a, None) for a in args]
    call[-1] = stream
    assert fn(*call) == 0, entry
    torch.cuda.synchronize()
    for i in outputs:
        assert not bool(torch.isnan(args[i].float()).any()), f"{entry}: output {i} of the valid call"


# ---------------------------------------------------------------------------------------------------------------
# Q. an optimiser slice riding on a link
# ---------------------------------------------------------------------------------------------------------------
def _rider_state(hip):
    r = LC.rider_case()
    s = {k: r[k].cuda() for k in ("p", "g", "ms", "mg", "mom")}
    s["lr"] = torch.tensor([LC.RIDER_HYPER["lr"]], dtype=torch.float32).cuda()
    h = LC.RIDER_HYPER
    s["slice"] = hip.rmsprop_slice(s["p"], s["g"], s["ms"], s["mg"], s["mom"], LC.RIDER_LO, LC.RIDER_HI, LC.RIDER_N, s["lr"], decay=h["decay"],
                                   momentum=h["momentum"], eps=h["eps"])
    return r, s


def _check_rider(r, s, tag):
    lo, hi = LC.RIDER_LO, LC.RIDER_HI
    for k, ref in zip(("p", "ms", "mg", "mom"), r["ref"]):
        assert_close(s[k][lo:hi], ref, *LC.RMS_TOL[k], tag + k + " of the slice", "Q")
        assert_bits(s[k][:lo], r[k][:lo], tag + k + " below the slice"); assert_bits(s[k][hi:], r[k][hi:], tag + k + " above the slice")
        assert not torch.equal(s[k][lo:hi].cpu(), r[k][lo:hi])
    assert_bits(s["g"], r["g"], tag + "the gradient")


def test_rider_on_the_4_wave_link(hip):
    M, Hd, layout, body = LC.RIDER_SHAPE
    assert LC.bwd_body(M, Hd, layout) == "kw4"
    c = LC.bwd_case(M, Hd, UNIT)
    tag = "rider on lstm_bwd_fused_kernel<4> "
    dgn, w_h, act, c_prev, cc = (dev(c[k]) for k in ("dgates_next", "w_h", "gate_act", "c_prev", "c"))
    dh_a, dh_b, dc_in = dev(c["dh_a"]), dev(c["dh_b"]), dev(c["dc_in"])
    r, s = _rider_state(hip)
    (b0, v0), (b1, v1) = out(M, 4 * Hd), out(M, Hd)
    dg, dcp = hip.lstm_step_bwd_opt(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc, s["slice"], out=(v0, v1))
    dg2, dcp2 = hip.lstm_step_bwd_opt(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc, None)
    dg3, dcp3, _ = hip.lstm_step_bwd(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc)
    torch.cuda.synchronize()
    tails((b0, b1), M, tag)
    for a, b_ in ((dg, dg2), (dcp, dcp2), (dg, dg3), (dcp, dcp3)):
        assert_bits(a, b_, tag + "the link with and without the slice")
    ref = LC.lstm_bwd64(c["dgates_next"], c["w_h"], c["dh_a"], c["dh_b"], c["dc_in"], c["gate_act"], c["c_prev"], c["c"])
    assert_close(dg, ref[0], *BWD_TOL, tag + "dgates", "Q"); assert_close(dcp, ref[1], *BWD_TOL, tag + "dc_prev", "Q")
    _check_rider(r, s, tag)


def test_rider_on_the_pointwise_backward(hip):
    M, Hd, regime = LC.PW_BWD_RUNS[1]
    c = LC.bwd_case(M, Hd, regime)
    tag = "rider on lstm_pw_bwd_opt_kernel "
    act, c_prev, cc, dh, dc = (dev(c[k]) for k in ("gate_act", "c_prev", "c", "dh_a", "dc_in"))
    r, s = _rider_state(hip)
    dg, dcp = hip.lstm_pointwise_bwd_opt(act, c_prev, cc, dh, dc, s["slice"])
    dg2, dcp2 = hip.lstm_pointwise_bwd(act, c_prev, cc, dh, dc)
    torch.cuda.synchronize()
    assert_bits(dg, dg2, tag + "dgates with and without the slice"); assert_bits(dcp, dcp2, tag + "dc_prev with and without the slice")
    ref = LC.lstm_bwd64(None, None, c["dh_a"], None, c["dc_in"], c["gate_act"], c["c_prev"], c["c"])
    assert_close(dg, ref[0], *BWD_TOL, tag + "dgates", "Q"); assert_close(dcp, ref[1], *BWD_TOL, tag + "dc_prev", "Q")
    _check_rider(r, s, tag)
