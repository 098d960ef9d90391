"""GPU tests of the half-tile forms (8 x 16 and 8 x 8 output tiles) of the 16-wave long-K launches: the BPTT kernels
lstm_bwd_fused_kernel<16> and lstm_bwd_entry_kernel, and the grouped long-K NT products of air_gemm_grouped
(gemm_grouped_longk_half_kernel; AIR_GEMM_LONGK_TILE, held to the bits of the 16 x 16 launch and to the float64 bound of
tests/gemm_cases.py in the same way).  Run with -m gpu on an MI355X.  A half tile keeps, for every output element, the accumulation chain of the
16 x 16 tile -- the same K chunks on the same waves, the same order inside a chunk, the same reduction over the waves -- so every
forced shape (AIR_LSTM_BWD_TILE, read at every call) is held to the BITS of the 16 x 16 launch, and the 16 x 16 launch to the float64
restatement of tests/lstm_cases.py at lstm_cases.BWD_TOL.  An optimiser slice riding on a half-tile grid is held to the bits of
air_rmsprop on the same elements, and a forced shape outside its domain to AIR_E_UNSUPPORTED with nothing written.

Inputs sit in buffers with two rows of NaN behind them, outputs start as NaN with two sentinel rows behind that are compared."""
import contextlib
import os

import pytest
import torch

import gemm_cases as GC
import lstm_cases as LC
from lstm_cases import BF16, BWD_TOL, F32, SENTINEL, UNIT, assert_bits, assert_close

pytestmark = pytest.mark.gpu
NAN = float("nan")
E_UNSUPPORTED = -5
ENV = "AIR_LSTM_BWD_TILE"
GEMM_ENV = "AIR_GEMM_LONGK_TILE"
HALF_SHAPES = ("8x16", "8x8")

# (M, Hd): one half tile; row and column tails inside the second half tiles (K = 48); K = 160: fewer chunks than waves; (24, 48);
# K = 1088: a second trip through the chunk loop
LINK_SHAPES = [(8, 8), (9, 12), (20, 40), (24, 48), (8, 272)]
# with and without dh_b, dc_in and dgx_in (lstm_cases.PATTERNS)
LINK_PATTERNS = ("all", "none")
# (M, Hd), Hd % 16 == 0; (24, 272): 17 unit chunks, a second loop trip
ENTRY_SHAPES = [(8, 16), (9, 48), (24, 272)]


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@contextlib.contextmanager
def tile(shape, env=ENV):
    """the developer switch for the calls inside: read by the library at every call, so one process runs every form"""
    before = os.environ.get(env)
    os.environ[env] = shape
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(env, None)
        else:
            os.environ[env] = before


def dev(t):
    """t[M, n] on the device as the first M rows of a buffer of M + 2 rows, the rest NaN"""
    if t is None:
        return None
    M, n = t.shape
    buf = torch.full((M + 2, n), NAN, dtype=torch.float32, device="cuda")
    buf[:M].copy_(t.cuda())
    return buf[:M]


def out(M, n):
    buf = torch.full((M + 2, n), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:M] = NAN
    return buf, buf[:M]


def tails(bufs, M, what):
    for i, b in enumerate(bufs):
        if b is not None:
            assert bool((b[M:] == SENTINEL).all()), f"{what}: output {i} written past row M"


def complete(t, what):
    assert bool(torch.isfinite(t).all()), what + ": elements left unwritten"


# ---------------------------------------------------------------------------------------------------------------
# the link
# ---------------------------------------------------------------------------------------------------------------
def _run_link(hip, c, pattern, shape, tag):
    M, Hd = c["M"], c["Hd"]
    dgn, w_h, act, c_prev, cc = (dev(c[k]) for k in ("dgates_next", "w_h", "gate_act", "c_prev", "c"))
    dh_a, dh_b, dc_in, dgx_src = (dev(t) for t in LC.pattern_operands(c, pattern))
    want_dgx = LC.PATTERNS[pattern][4]
    (bd, vd), (bc, vc) = out(M, 4 * Hd), out(M, Hd)
    bx, vx = out(M, 4 * Hd) if want_dgx else (None, None)
    with tile(shape):
        dg, dcp, dgx = hip.lstm_step_bwd(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc, dgx_in=dgx_src, out=(vd, vc, vx))
    torch.cuda.synchronize()
    tails((bd, bc, bx), M, tag)
    complete(dg, tag + "dgates"); complete(dcp, tag + "dc_prev")
    if dgx is not None:
        complete(dgx, tag + "dgx")
    return dg, dcp, dgx


@pytest.mark.parametrize("shape", LINK_SHAPES, ids=str)
def test_link_half_tiles_repeat_the_bits_of_the_full_tile(hip, shape):
    M, Hd = shape
    assert LC.bwd_body(M, Hd, "") == "kw16"
    c = LC.bwd_case(M, Hd, UNIT)
    for pattern in LINK_PATTERNS:
        tag = f"link {shape} {pattern} "
        full = _run_link(hip, c, pattern, "16x16", tag + "16x16 ")
        ref = LC.bwd_ref(M, Hd, UNIT, F32, pattern)
        for got, r, nm in zip(full, ref, ("dgates", "dc_prev", "dgx")):
            if got is None:
                assert not LC.PATTERNS[pattern][4] and nm == "dgx"
            else:
                assert_close(got, r, *BWD_TOL, tag + nm + " of the 16x16 launch against float64")
        auto = _run_link(hip, c, pattern, "auto", tag + "auto ")
        for form, res in [(s, _run_link(hip, c, pattern, s, tag + s + " ")) for s in HALF_SHAPES] + [("auto", auto)]:
            for got, want, nm in zip(res, full, ("dgates", "dc_prev", "dgx")):
                assert (got is None) == (want is None)
                if got is not None:
                    assert_bits(got, want, tag + nm + f": {form} against 16x16")


# ---------------------------------------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------------------------------------
def _run_entry(hip, d, M, Hd, shape, tag, opt=None):
    pairs = [out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd)]
    bufs, views = zip(*pairs)
    with tile(shape):
        res = hip.lstm_step_bwd_entry(d["act1"], d["c1"], d["c2"], d["dh_a1"], d["dh_b1"], d["w_h"], d["dh_a0"], d["dh_b0"], d["act0"], d["c0"],
                                      d["c1"], opt=opt, out=views)
    torch.cuda.synchronize()
    tails(bufs, M, tag)
    for t, nm in zip(res, ("dgates1", "dc_prev1", "dgates", "dc_prev", "dgx")):
        complete(t, tag + nm)
    return res


@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=str)
def test_entry_half_tiles_repeat_the_bits_of_the_full_tile(hip, shape):
    M, Hd = shape
    c = LC.entry_case(M, Hd, UNIT)
    d = {k: dev(c[k]) for k in ("act1", "act0", "c0", "c1", "c2", "dh_a1", "dh_b1", "dh_a0", "dh_b0", "w_h")}
    names = ("dgates1", "dc_prev1", "dgates", "dc_prev", "dgx")
    tag = f"entry {shape} "
    full = _run_entry(hip, d, M, Hd, "16x16", tag + "16x16 ")
    for got, r, nm in zip(full, LC.entry_ref(c, "all"), names):
        assert_close(got, r, *BWD_TOL, tag + nm + " of the 16x16 launch against float64")
    for form in HALF_SHAPES + ("auto", "link=16x16,entry=8x8"):
        res = _run_entry(hip, d, M, Hd, form, tag + form + " ")
        for got, want, nm in zip(res, full, names):
            assert_bits(got, want, tag + nm + f": {form} against 16x16")


# ---------------------------------------------------------------------------------------------------------------
# an optimiser slice riding on a half-tile grid
# ---------------------------------------------------------------------------------------------------------------
def _rider(hip):
    """the riding slice of lstm_cases.rider_case, and what air_rmsprop makes of the same elements"""
    r = LC.rider_case()
    s = {k: r[k].cuda() for k in ("p", "g", "ms", "mg", "mom")}
    s["lr"] = torch.tensor([LC.RIDER_HYPER["lr"]], dtype=torch.float32).cuda()
    h = LC.RIDER_HYPER
    s["slice"] = hip.rmsprop_slice(s["p"], s["g"], s["ms"], s["mg"], s["mom"], LC.RIDER_LO, LC.RIDER_HI, LC.RIDER_N, s["lr"], decay=h["decay"],
                                   momentum=h["momentum"], eps=h["eps"])
    lo, hi = LC.RIDER_LO, LC.RIDER_HI
    want = {k: r[k][lo:hi].clone().cuda() for k in ("p", "g", "ms", "mg", "mom")}
    hip.rmsprop_centered_(want["p"], want["g"], want["ms"], want["mg"], want["mom"], s["lr"], decay=h["decay"], momentum=h["momentum"],
                          eps=h["eps"])
    torch.cuda.synchronize()
    return r, s, want


def _check_rider(r, s, want, tag):
    lo, hi = LC.RIDER_LO, LC.RIDER_HI
    for k in ("p", "ms", "mg", "mom"):
        assert_bits(s[k][lo:hi], want[k], tag + k + " of the slice against air_rmsprop")
        assert_bits(s[k][:lo], r[k][:lo], tag + k + " below the slice"); assert_bits(s[k][hi:], r[k][hi:], tag + k + " above the slice")
        assert not torch.equal(s[k][lo:hi].cpu(), r[k][lo:hi])
    assert_bits(s["g"], r["g"], tag + "the gradient")


def test_rider_on_a_half_tile_link(hip):
    M, Hd = 24, 48                      # 8x16: 3 x 3 tiles, the rider workgroups start at block 9 (16x16: 2 x 3, block 6)
    c = LC.bwd_case(M, Hd, UNIT)
    tag = "rider on lstm_bwd_fused_kernel<16> at 8x16 "
    dgn, w_h, act, c_prev, cc = (dev(c[k]) for k in ("dgates_next", "w_h", "gate_act", "c_prev", "c"))
    dh_a, dh_b, dc_in = dev(c["dh_a"]), dev(c["dh_b"]), dev(c["dc_in"])
    r, s, want = _rider(hip)
    (b0, v0), (b1, v1) = out(M, 4 * Hd), out(M, Hd)
    with tile("8x16"):
        dg, dcp = hip.lstm_step_bwd_opt(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc, s["slice"], out=(v0, v1))
    with tile("16x16"):
        dg2, dcp2 = hip.lstm_step_bwd_opt(dgn, w_h, dh_a, dh_b, dc_in, act, c_prev, cc, None)
    torch.cuda.synchronize()
    tails((b0, b1), M, tag)
    assert_bits(dg, dg2, tag + "dgates against the 16x16 link without a slice")
    assert_bits(dcp, dcp2, tag + "dc_prev against the 16x16 link without a slice")
    _check_rider(r, s, want, tag)


def test_rider_on_a_half_tile_entry(hip):
    M, Hd = 9, 48                       # 8x8: 2 x 6 tiles, the rider workgroups start at block 12 (16x16: 1 x 3, block 3)
    c = LC.entry_case(M, Hd, UNIT)
    d = {k: dev(c[k]) for k in ("act1", "act0", "c0", "c1", "c2", "dh_a1", "dh_b1", "dh_a0", "dh_b0", "w_h")}
    tag = "rider on lstm_bwd_entry_kernel at 8x8 "
    r, s, want = _rider(hip)
    res = _run_entry(hip, d, M, Hd, "8x8", tag, opt=s["slice"])
    full = _run_entry(hip, d, M, Hd, "16x16", tag + "16x16 ")
    for got, w_, nm in zip(res, full, ("dgates1", "dc_prev1", "dgates", "dc_prev", "dgx")):
        assert_bits(got, w_, tag + nm + " against the 16x16 entry without a slice")
    _check_rider(r, s, want, tag)


# ---------------------------------------------------------------------------------------------------------------
# a forced shape outside its domain
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [(2049, 50, F32, "8x8"), (2049, 64, F32, "8x16"), (24, 48, BF16, "8x16"), (24, 48, F32, "4x4"),
                                 (2049, 50, F32, "entry=16x16,link=8x16"), (24, 48, F32, "link=8x16,entry=7x7")], ids=str)
def test_forced_shape_outside_its_domain_is_refused(hip, run):
    """half tiles exist for the 16-wave fp32 link only: the 4-wave and wide-tile links (more than 512 tiles of 16 x 16), the bf16
    operand mode and a shape the switch does not know (also in its "launch=shape" list form) return AIR_E_UNSUPPORTED and write
    nothing"""
    from attend_infer_repeat_amd import _lib
    M, Hd, precision, shape = run
    if M > 2048:
        assert LC.bwd_body(M, Hd, "") != "kw16"
    c = LC.bwd_case(M, Hd, UNIT)
    dgn, w_h, act, c_prev, cc = (dev(c[k]) for k in ("dgates_next", "w_h", "gate_act", "c_prev", "c"))
    (bd, vd), (bc, vc), (bx, vx) = out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd)
    for b in (bd, bc, bx):
        b.fill_(SENTINEL)
    with tile(shape):
        with pytest.raises(_lib.AirHipError) as err:
            hip.lstm_step_bwd(dgn, w_h, None, None, None, act, c_prev, cc, precision=precision, out=(vd, vc, vx))
    torch.cuda.synchronize()
    assert f"status {E_UNSUPPORTED}:" in str(err.value), str(err.value)
    for b in (bd, bc, bx):
        assert bool((b == SENTINEL).all()), f"{run}: a refused launch wrote"
    if M > 2048:                                       # the same call goes through once the switch is back on auto
        with tile("auto"):
            hip.lstm_step_bwd(dgn, w_h, None, None, None, act, c_prev, cc, precision=precision, out=(vd, vc, vx))
        torch.cuda.synchronize()
        complete(vd, f"{run} auto dgates")


def test_forced_shape_the_entry_cannot_honour_is_refused(hip):
    from attend_infer_repeat_amd import _lib
    M, Hd = 9, 48
    c = LC.entry_case(M, Hd, UNIT)
    d = {k: dev(c[k]) for k in ("act1", "act0", "c0", "c1", "c2", "dh_a1", "dh_b1", "dh_a0", "dh_b0", "w_h")}
    pairs = [out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd), out(M, Hd), out(M, 4 * Hd)]
    bufs, views = zip(*pairs)
    for b in bufs:
        b.fill_(SENTINEL)
    with tile("16x8"):
        with pytest.raises(_lib.AirHipError) as err:
            hip.lstm_step_bwd_entry(d["act1"], d["c1"], d["c2"], d["dh_a1"], d["dh_b1"], d["w_h"], d["dh_a0"], d["dh_b0"], d["act0"], d["c0"], d["c1"],
                                    out=views)
    torch.cuda.synchronize()
    assert f"status {E_UNSUPPORTED}:" in str(err.value), str(err.value)
    for b in bufs:
        assert bool((b == SENTINEL).all()), "a refused entry launch wrote"


# ---------------------------------------------------------------------------------------------------------------
# the grouped long-K launch
# ---------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(9, 24, 528), (20, 40, 1040)]       # (M, N, K), both NT: row and column tails inside half tiles; 33 and 65 K chunks for 16 waves


def _gemm_problem(seed, M, N, K, epi):
    """operands with the magnitudes of tests/gemm_cases.py (|x| in [0.5, 1.5], random signs), the float64 result and its bound
    CONST["S"] 2^-24 (S + |out64|), S = sum_k |a b| (gemm_cases.data / bound for the NONE and MUL_DELU epilogues)"""
    gen = torch.Generator().manual_seed(seed)
    a, b = GC._signed(gen, M, K), GC._signed(gen, N, K)
    aux = GC._elu_output(gen, M, N) if epi == GC.EPI_MUL_DELU else None
    acc = a.double() @ b.double().t()
    out64 = acc * GC.elu_prime(aux.double()) if aux is not None else acc
    bound = GC.CONST["S"] * GC.U32 * (a.double().abs() @ b.double().abs().t() + out64.abs())
    return dict(a=a, b=b, aux=aux, epi=epi, out64=out64, bound=bound, M=M, N=N)


def _run_gemm(hip, probs, shape, tag):
    bufs, descs = [], []
    for p in probs:
        buf, view = out(p["M"], p["N"])
        bufs.append(buf)
        d = dict(A=dev(p["a"]), B=dev(p["b"]), tb=True, epilogue=p["epi"], out=view)
        if p["aux"] is not None:
            d["aux"] = dev(p["aux"])
        descs.append(d)
    with tile(shape, GEMM_ENV):
        res = [c for c, _ in hip.gemm_grouped(descs)]
    torch.cuda.synchronize()
    for p, b, c in zip(probs, bufs, res):
        tails((b,), p["M"], tag)
        complete(c, tag + "C")
    return res


@pytest.mark.parametrize("epis", [(GC.EPI_NONE, GC.EPI_MUL_DELU), (GC.EPI_MUL_DELU, GC.EPI_NONE)], ids=["none+mdelu", "mdelu+none"])
def test_grouped_long_k_half_tiles_repeat_the_bits_of_the_full_tile(hip, epis):
    probs = [_gemm_problem(1000 + 7 * i + e, M, N, K, e) for i, ((M, N, K), e) in enumerate(zip(GEMM_SHAPES, epis))]
    tag = f"grouped long-K {epis} "
    full = _run_gemm(hip, probs, "16x16", tag + "16x16 ")
    for i, (p, c) in enumerate(zip(probs, full)):
        err = (c.double().cpu() - p["out64"]).abs()
        worst = float((err / p["bound"]).max())
        print(f"{tag}problem {i}: worst error / bound of the 16x16 launch {worst:.3f}")
        assert worst <= 1.0, f"{tag}problem {i}: {worst} of the float64 bound"
    for form in HALF_SHAPES + ("auto",):
        for i, (c, want) in enumerate(zip(_run_gemm(hip, probs, form, tag + form + " "), full)):
            assert_bits(c, want, tag + f"problem {i}: {form} against 16x16")


@pytest.mark.parametrize("what", ["tn", "bias", "bf16", "4x4"])
def test_forced_long_k_shape_outside_its_domain_is_refused(hip, what):
    """a 16-wave launch with a problem that is no NT product, has another epilogue or bf16 operands, and a value the switch does not
    know: AIR_E_UNSUPPORTED, nothing written; on auto the same launch goes through"""
    from attend_infer_repeat_amd import _lib
    gen = torch.Generator().manual_seed(77)
    M, N, K = 9, 24, 528
    a, b = GC._signed(gen, M, K), GC._signed(gen, N, K)
    buf, view = out(M, N)
    buf.fill_(SENTINEL)
    d = dict(A=dev(a), B=dev(b), tb=True, out=view)
    if what == "tn":
        d = dict(A=dev(a.t().contiguous()), B=dev(b.t().contiguous()), ta=True, out=view)
    elif what == "bias":
        d.update(epilogue=hip.EPI_BIAS, bias=torch.ones(N, device="cuda"))
    with tile("4x4" if what == "4x4" else "8x16", GEMM_ENV):
        with pytest.raises(_lib.AirHipError) as err:
            hip.gemm_grouped([d], precision=BF16 if what == "bf16" else F32)
    torch.cuda.synchronize()
    assert f"status {E_UNSUPPORTED}:" in str(err.value), str(err.value)
    assert bool((buf == SENTINEL).all()), f"{what}: a refused launch wrote"
    with tile("auto", GEMM_ENV):
        hip.gemm_grouped([d], precision=BF16 if what == "bf16" else F32)
    torch.cuda.synchronize()
    complete(view, f"{what} auto C")
