"""GPU parity of the launches folded into the train step, one launch at a time (run with -m gpu on an MI355X): the closing update in
the weight-gradient tiles (air_gemm_grouped_opt), the Gaussian head's backward in the decoder's dX epilogue
(air_gemm_grouped_gauss_bwd), the HBM feeder on its own, in the A-operand load of the first products and in the step prologue, the
step prologue on its own and riding on the first LSTM step with and without the hoisted input product, and the small riders of the
canvas backward, the share sums, the L2 term and the step counter.

Cases and float64 references come from tests/fold_cases.py (built and cross-checked on the CPU by tests/test_fold_cases_host.py).
Every output buffer starts as NaN, every buffer a launch must not touch as a sentinel that is compared for bits afterwards.  Each
folded launch is held twice: against float64 at the bound the unfused kernel's own test uses, and bit for bit against the launches it
replaces.  A reference that depends on an intermediate the launch writes (the update on the gradient, the head's backward on the
sample gradient, the step on gx) is evaluated on the written value, which is checked against float64 on its own.

Group letters (G folded update, H Gaussian backward, I feeder, J prologue / first LSTM step, K small riders) tag every comparison;
the worst error / tolerance ratio of each group is printed when the module finishes (pytest -s)."""
import ctypes

import pytest
import torch

import fold_cases as FC
from fold_cases import SENTINEL, assert_bits, assert_close, g, print_worst
from test_objective_kernels import _check_nvil, _nvil_ref

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print_worst("fold kernels", "GHIJK")


def i64(*v):
    return torch.tensor(list(v), dtype=torch.int64).cuda()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def padded(rows, cols, ld, fill=NAN):
    """a [rows, cols] view (filled with `fill`) of a [rows, ld] buffer whose padding columns hold the sentinel"""
    buf = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:, :cols] = fill
    return buf, buf[:, :cols]


def assert_padding(buf, cols, what):
    assert bool((buf[:, cols:] == SENTINEL).all()), what + ": padding columns written"


# ---------------------------------------------------------------------------------------------------------------
# G. air_gemm_grouped_opt
# ---------------------------------------------------------------------------------------------------------------
STEP0, OFFSET0 = 41, 1000


def _opt_state(c):
    """device copies of the flat buffers (the folded regions of g NaN-primed), the counters and the problems of the case"""
    s = {k: g(c[k]) for k in ("p", "g", "ms", "mg", "mom")}
    for lo, hi in c["fold_regions"]:
        s["g"][lo:hi] = NAN
    s["lr"] = torch.tensor([c["lr"]], dtype=torch.float32).cuda()
    s["step"], s["rng"] = i64(STEP0), i64(77, OFFSET0)
    s["problems"] = []
    for i, pr in enumerate(c["problems"]):
        d = dict(A=g(pr["X"]), B=g(pr["dY"]), ta=True)
        if pr["folded"]:
            lo = c["c_off"][i]
            d["out"] = s["g"][lo:lo + pr["M"] * pr["N"]].view(pr["M"], pr["N"])
            if pr["colsum"]:
                d["colsum"] = s["g"][c["cs_off"][i]:c["cs_off"][i] + pr["N"]]
        else:
            d["out"] = nans(pr["M"], pr["N"])
            if pr["colsum"]:
                d["colsum"] = nans(pr["N"])
        s["problems"].append(d)
    return s


def _opt_fold(hip, c, s):
    kw = dict(lr_mult_tail=c["lr_mult_tail"], decay=c["decay"], momentum=c["momentum"], eps=c["eps"], grad_scale=c["grad_scale"])
    if c["counters"]:
        kw.update(global_step_dev=s["step"], rng_state_dev=s["rng"], rng_increment=FC.RNG_INCREMENT)
    return hip.opt_fold(s["p"], s["g"], s["ms"], s["mg"], s["mom"], c["n_model"], s["lr"], c["fold_mask"], c["ranges"], **kw)


def _opt_unfolded(hip, c, s):
    """air_gemm_grouped, then air_step_epilogue over every region the folded launch updates (the counters with the first one)"""
    hip.gemm_grouped(s["problems"], precision=c["precision"])
    first = True
    for lo, hi in c["fold_regions"] + c["ranges"]:
        if hi == lo:
            continue
        kw = dict(global_step_dev=s["step"], rng_state_dev=s["rng"], rng_increment=FC.RNG_INCREMENT) if (first and c["counters"]) else {}
        first = False
        hip.step_epilogue_(s["p"][lo:hi], s["g"][lo:hi], s["ms"][lo:hi], s["mg"][lo:hi], s["mom"][lo:hi], min(max(c["n_model"] - lo, 0), hi - lo),
                           s["lr"], c["lr_mult_tail"], c["decay"], c["momentum"], c["eps"], c["grad_scale"], **kw)


@pytest.mark.parametrize("name,precision", FC.OPT_RUNS)
def test_gemm_grouped_opt(hip, name, precision):
    c = FC.opt_case(name, precision)
    tag = f"opt {name} prec={precision} "
    a, b = _opt_state(c), _opt_state(c)
    st, outs = hip.gemm_grouped_opt(a["problems"], _opt_fold(hip, c, a), precision=precision)
    assert st == 0, tag + "status"
    _opt_unfolded(hip, c, b)
    torch.cuda.synchronize()
    # 1. everything against air_gemm_grouped + air_step_epilogue, bit for bit
    for k in ("p", "g", "ms", "mg", "mom", "step", "rng"):
        assert_bits(a[k], b[k], tag + k + " against the unfolded launches")
    for i, pr in enumerate(c["problems"]):
        if not pr["folded"]:
            assert_bits(outs[i][0], b["problems"][i]["out"], tag + f"unfolded dW[{i}]")
    # 2. the gradients against the float64 products
    for i, pr in enumerate(c["problems"]):
        rtol, atol = FC.product_tol(pr["K"])
        assert_close(outs[i][0], pr["C64"], rtol, atol, tag + f"dW[{i}]", "G")
        if pr["colsum"]:
            assert_close(outs[i][1], pr["colsum64"], rtol, atol, tag + f"colsum[{i}]", "G")
    # 3. the update against float64 RMSProp of the gradient the launch wrote
    t = c["touched"]
    gw = a["g"].cpu()
    assert bool(torch.isfinite(gw[t]).all())
    ref = FC.rmsprop64(c["p"][t], gw[t], c["ms"][t], c["mg"][t], c["mom"][t], c["lr_elem"][t], c["decay"], c["momentum"], c["eps"], c["grad_scale"])
    for k, r in zip(("p", "ms", "mg", "mom"), ref):
        assert_close(a[k].cpu()[t], r, *FC.RMS_TOL[k], tag + k, "G")
        assert_bits(a[k].cpu()[~t], c[k][~t], tag + k + " outside the regions")
    assert_bits(gw[~t], c["g"][~t], tag + "g outside the folded problems")
    for lo, hi in c["ranges"]:
        assert_bits(gw[lo:hi], c["g"][lo:hi], tag + "g of a rider range")
    if c["counters"]:
        assert a["step"].tolist() == [STEP0 + 1] and a["rng"].tolist() == [77, OFFSET0 + FC.RNG_INCREMENT], tag + "counters"
    else:
        assert a["step"].tolist() == [STEP0] and a["rng"].tolist() == [77, OFFSET0], tag + "counters of the early fold"


@pytest.mark.parametrize("name", sorted(FC.OPT_DECLINED))
def test_gemm_grouped_opt_declines_and_writes_nothing(hip, name):
    c = FC.opt_case(name, FC.F32, True)
    a, before = _opt_state(c), _opt_state(c)
    st, _ = hip.gemm_grouped_opt(a["problems"], _opt_fold(hip, c, a))
    torch.cuda.synchronize()
    assert st == hip.E_UNSUPPORTED
    for k in ("p", "g", "ms", "mg", "mom", "step", "rng"):
        assert_bits(a[k], before[k], f"declined {name}: {k}")


# ---------------------------------------------------------------------------------------------------------------
# H. air_gemm_grouped_gauss_bwd
# ---------------------------------------------------------------------------------------------------------------
def _gb_problems(hip, c):
    ds = dict(A=g(c["gy"]), B=g(c["W"]), tb=True, out=nans(c["M"], c["D"]))
    if not c["others"]:
        return [ds]
    tn, nt = c["others"]
    return [dict(A=g(tn["A"]), B=g(tn["B"]), ta=True, out=nans(33, 20)), ds,
            dict(A=g(nt["A"]), B=g(nt["B"]), tb=True, epilogue=hip.EPI_MUL_DELU, aux=g(nt["aux"]), out=nans(21, 70))]


def _gb_riders(c):
    nv = None
    if c["nvil"] is not None:
        nv = dict(imp_parts=g(c["imp_parts"]), baseline=g(c["baseline"]), logp=g(c["logp"]), ema=g(c["ema"]))
    return nv, (g(c["kl_parts"]) if c["n_kl"] else None)


@pytest.mark.parametrize("i", range(len(FC.GB_RUNS)))
def test_gemm_grouped_gauss_bwd(hip, i):
    c = FC.gb_case(i)
    M, D, K = c["M"], c["D"], c["K"]
    tag = f"gauss_bwd case {i} "
    pre_buf, pre = padded(M, 2 * D, c["ld_pre"], 0.0)
    pre.copy_(g(c["pre"]))
    eps, loc, scale, dkl = g(c["eps"]), g(c["loc"]), g(c["scale"]), g(c["dkl_row"])
    common = (pre, eps, FC.GB_OFFSET, FC.GB_PRIOR, loc, scale)
    # the folded launch
    probs_a = _gb_problems(hip, c)
    dbuf_a, dpre_a = padded(M, 2 * D, c["ld_dpre"])
    nv_a, kl_a = _gb_riders(c)
    st, outs, rid_a = hip.gemm_grouped_gauss_bwd(probs_a, c["problem"], *common, dkl, FC.GB_DKL_SCALE, dpre_a, c["guard"], c["precision"], nv_a, kl_a)
    assert st == 0
    # the launches it replaces
    probs_b = _gb_problems(hip, c)
    dbuf_b, dpre_b = padded(M, 2 * D, c["ld_dpre"])
    nv_b, kl_b = _gb_riders(c)
    outs_b = hip.gemm_grouped(probs_b, precision=c["precision"])
    rid_b = hip.gauss_sample_bwd_nvil(*common, outs_b[c["problem"]][0], dkl, FC.GB_DKL_SCALE, dpre_b, c["guard"], nv_b, kl_b)
    torch.cuda.synchronize()
    dsample = outs[c["problem"]][0]
    assert_close(dsample, c["dsample64"], *FC.product_tol(K), tag + "dsample", "H")
    for j, o in enumerate(c["others"]):
        assert_close(outs[0 if j == 0 else 2][0], o["ref"], *FC.product_tol(o["K"]), tag + o["kind"], "H")
    ref = FC.gauss_dpre64(c["pre"], c["eps"], dsample.cpu(), c["dkl_row"], c["guard"])
    assert_close(dpre_a, ref, 1e-4, 1e-5, tag + "dpre", "H")
    assert_padding(dbuf_a, 2 * D, tag + "dpre"); assert_padding(pre_buf, 2 * D, tag + "pre")
    if c["nvil"] is not None:
        total = FC.sum_in_order32(c["imp_parts"])
        assert_bits(rid_a["imp_sum"].cpu(), total, tag + "imp_sum")
        mm, mv, d = (float(v) for v in c["ema"][:3])
        rout, rdlogp, rdbase, raw_mean, raw_var = _nvil_ref(total, c["baseline"], c["logp"], ema=(mm, mv))
        _check_nvil((rid_a["out"], rid_a["dlogp"], rid_a["dbaseline"]), (rout, rdlogp, rdbase), tag + "nvil ", group="H")
        assert_close(nv_a["ema"][:2], torch.stack([d * mm + (1 - d) * raw_mean, d * mv + (1 - d) * raw_var]), 1e-5, 0.0, tag + "averages", "H")
        assert_bits(nv_a["ema"], nv_b["ema"], tag + "moving averages against the unfused launch")
    if c["n_kl"]:
        assert_bits(rid_a["kl_row"].cpu(), FC.sum_in_order32(c["kl_parts"]), tag + "kl_row_out")
        assert_close(rid_a["kl_row"], c["kl_parts"].double().sum(0), 1e-6, 0.0, tag + "kl_row_out", "H")
    assert set(rid_a) == set(rid_b)
    for k in rid_a:
        assert_bits(rid_a[k], rid_b[k], tag + k + " against the unfused launch")
    assert_bits(dbuf_a, dbuf_b, tag + "dpre against the unfused launch")
    for (oa, _), (ob, _) in zip(outs, outs_b):
        assert_bits(oa, ob, tag + "products against air_gemm_grouped")


def test_gemm_grouped_gauss_bwd_declines_more_than_1000_tiles(hip):
    f = FC.GB_DECLINED
    M, D, K = f["M"], f["D"], f["K"]
    em, en, ek = f["extra"]
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    probs = [dict(A=rnd(M, K), B=rnd(D, K), tb=True, out=nans(M, D)), dict(A=rnd(ek, em), B=rnd(ek, en), ta=True, out=nans(em, en))]
    dpre = nans(M, 2 * D)
    st, outs, _ = hip.gemm_grouped_gauss_bwd(probs, 0, rnd(M, 2 * D), rnd(M, D), FC.GB_OFFSET, FC.GB_PRIOR, rnd(M, D), rnd(M, D).abs() + 0.1, None,
                                             0.0, dpre)
    torch.cuda.synchronize()
    assert st == hip.E_UNSUPPORTED
    assert bool(torch.isnan(dpre).all()) and all(bool(torch.isnan(o).all()) for o, _ in outs)


# ---------------------------------------------------------------------------------------------------------------
# I. the feeder
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(FC.GATHER_CASES)))
def test_batch_gather(hip, i):
    c = FC.gather_case(i)
    B, n = c["B"], c["item_floats"]
    data = g(c["data"])
    buf = torch.full((B * n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[:B * n].view(B, n)
    out.fill_(NAN)
    seed, step = i64(FC.FEED_SEED), i64(c["step"])
    _, idx = hip.batch_gather(data, seed, step, c["shuffle"], B, out=out)
    torch.cuda.synchronize()
    assert idx.tolist() == c["idx"], f"batch_gather case {i}: indices"
    assert_bits(out.cpu(), c["data"][torch.tensor(c["idx"])], f"batch_gather case {i}: rows")
    assert bool((buf[B * n:] == SENTINEL).all()) and seed.tolist() == [FC.FEED_SEED] and step.tolist() == [c["step"]]
    _, none = hip.batch_gather(data, seed, step, c["shuffle"], B, out=out, want_idx=False)          # idx_out == NULL
    assert none is None


def _gg_run(hip, c, folded):
    data = g(c["data"])
    seed, step = i64(FC.FEED_SEED), i64(FC.GG_STEP)
    obs = torch.full((c["B"], FC.GG_ITEMS), SENTINEL, dtype=torch.float32, device="cuda")
    idx = torch.full((c["B"],), -1, dtype=torch.int64, device="cuda") if (c["has_idx"] or not folded) else None
    outs = [padded(c["B"], p["N"], p["N"] + 4) for p in c["problems"]]
    if not folded:
        hip.batch_gather(data, seed, step, True, c["B"], out=obs)
    probs = [dict(A=obs[:, p["off"]:p["off"] + p["K"]], B=g(p["w"]), bias=g(p["bias"]), epilogue=hip.EPI_BIAS, out=o[1])
             for p, o in zip(c["problems"], outs)]
    if folded:
        bg = hip.batch_gather_desc(data, seed, step, True, obs, idx, c["copy_mask"])
        assert hip.gemm_grouped_gather_fits(probs, bg) == 1
        st, _ = hip.gemm_grouped_gather(probs, bg)
        assert st == 0
    else:
        hip.gemm_grouped(probs)
    torch.cuda.synchronize()
    return obs, idx, outs


@pytest.mark.parametrize("i", range(len(FC.GG_CASES)))
def test_gemm_grouped_gather(hip, i):
    c = FC.gg_case(i)
    tag = f"gather case {i} "
    obs, idx, outs = _gg_run(hip, c, True)
    obs_b, _, outs_b = _gg_run(hip, c, False)
    if c["has_idx"]:
        assert idx.tolist() == c["idx"], tag + "indices"
    cov = c["covered"]
    assert_bits(obs.cpu()[:, cov], c["obs"][:, cov], tag + "obs")
    assert bool((obs.cpu()[:, ~cov] == SENTINEL).all()), tag + "obs columns of no problem of copy_mask"
    assert_bits(obs_b.cpu(), c["obs"], tag + "obs of air_batch_gather")
    for p, (buf, out), (buf_b, out_b) in zip(c["problems"], outs, outs_b):
        assert_close(out, p["ref"], *FC.product_tol(p["K"]), tag + f"product at column {p['off']}", "I")
        assert_padding(buf, p["N"], tag + "product")
        assert_bits(buf, buf_b, tag + f"product at column {p['off']} against air_batch_gather + air_gemm_grouped")


def _fits_call(hip, change, obs, data, seed, step):
    from attend_infer_repeat_amd import _lib
    descs, bg = FC.fits_launch(change, obs=obs.data_ptr(), dataset=data.data_ptr())
    arr = (_lib.AirGemmDesc * 1)(*descs)
    gather = _lib.AirBatchGather(bg["dataset"], 37, bg["item_floats"], 1, bg["B"], seed.data_ptr(), step.data_ptr(), bg["obs"], None, 1)
    return arr, gather


def test_gemm_grouped_gather_fits_one_reason_at_a_time(hip):
    """the B operand and C of these descriptors are made-up addresses: the rule never reads them, and a declined launch starts nothing"""
    obs = torch.full((256, 2504), SENTINEL, dtype=torch.float32, device="cuda")
    data = torch.zeros(37 * 2504 + 4, dtype=torch.float32, device="cuda")
    seed, step = i64(FC.FEED_SEED), i64(3)
    L = hip.lib()
    for name, change in FC.FITS_ACCEPTED.items():
        arr, gather = _fits_call(hip, change, obs, data, seed, step)
        assert L.air_gemm_grouped_gather_fits(arr, 1, ctypes.byref(gather)) == 1, name
    for name, change in FC.FITS_DECLINED.items():
        arr, gather = _fits_call(hip, change, obs, data, seed, step)
        assert L.air_gemm_grouped_gather_fits(arr, 1, ctypes.byref(gather)) == 0, name
        assert L.air_gemm_grouped_gather(arr, 1, ctypes.byref(gather), hip._stream()) == hip.E_UNSUPPORTED, name
    torch.cuda.synchronize()
    assert bool((obs == SENTINEL).all())


@pytest.mark.parametrize("B,N,K", [(128, 256, 512), (256, 256, 1252)])
def test_gather_declines_a_group_air_gemm_grouped_runs_on_the_four_wave_body(hip, B, N, K):
    """The open question of the fits rule, decided: such a group met K >= 512 and the 1024-tile limit, ran on the gather's 16-wave
    K-split body, and air_gemm_grouped ran the same product on the 4-wave body (K < 8 min(M, N)): other partial sums, other bits
    (measured before the rule changed: 28 299 of 32 768 elements at (128, 256, 512), |difference| up to 1.4e-6).  The rule now
    asks for group_long_k as well, the launch declines, and the engine plans air_batch_gather + air_gemm_grouped."""
    gen = torch.Generator().manual_seed(B + K)
    data = torch.rand(37, K, generator=gen).cuda()
    w = (torch.randn(K, N, generator=gen) / K ** 0.5).cuda()
    seed, step = i64(FC.FEED_SEED), i64(3)
    obs = torch.full((B, K), SENTINEL, dtype=torch.float32, device="cuda")
    out = nans(B, N)
    bg = hip.batch_gather_desc(data, seed, step, True, obs, None, 1)
    probs = [dict(A=obs, B=w, out=out)]
    assert hip.gemm_grouped_gather_fits(probs, bg) == 0
    st, _ = hip.gemm_grouped_gather(probs, bg)
    torch.cuda.synchronize()
    assert st == hip.E_UNSUPPORTED and bool((obs == SENTINEL).all()) and bool(torch.isnan(out).all())
    # the two launches the engine plans instead
    hip.batch_gather(data, seed, step, True, B, out=obs)
    hip.gemm_grouped(probs)
    torch.cuda.synchronize()
    idx = torch.tensor(FC.feeder_indices(FC.FEED_SEED, 3, B, 37, True))
    assert_bits(obs.cpu(), data.cpu()[idx], "obs")
    assert_close(out, obs.double().cpu() @ w.double().cpu(), *FC.product_tol(K), f"product {B}x{N}x{K}", "I")


def _lone_gather(hip, B, N, K):
    """a lone NN product over rows of K floats drawn from 37 items: the launch's arguments, every output primed"""
    gen = torch.Generator().manual_seed(B + N + K)
    data = torch.rand(37, K, generator=gen).cuda()
    w = (torch.randn(K, N, generator=gen) / K ** 0.5).cuda()
    seed, step = i64(FC.FEED_SEED), i64(3)
    obs = torch.full((B, K), SENTINEL, dtype=torch.float32, device="cuda")
    buf, out = padded(B, N, N + 4)
    bg = hip.batch_gather_desc(data, seed, step, True, obs, None, 1)
    rows = data.cpu()[torch.tensor(FC.feeder_indices(FC.FEED_SEED, 3, B, 37, True))]
    return data, w, seed, step, obs, buf, out, bg, rows


def test_gather_takes_1000_tiles_bit_equal_to_the_two_launches(hip):
    """wide_min_tiles() tiles, the most the rule takes: air_gemm_grouped still runs the product on the 16-wave K split (its wide-tile
    regime starts one tile further), so the gather's product is that of air_batch_gather + air_gemm_grouped, bit for bit"""
    B, N, K = FC.GG_EDGE_TAKEN
    data, w, seed, step, obs, buf, out, bg, rows = _lone_gather(hip, B, N, K)
    probs = [dict(A=obs, B=w, out=out)]
    assert hip.gemm_grouped_gather_fits(probs, bg) == 1
    st, _ = hip.gemm_grouped_gather(probs, bg)
    assert st == 0
    obs_b = torch.full((B, K), SENTINEL, dtype=torch.float32, device="cuda")
    buf_b, out_b = padded(B, N, N + 4)
    hip.batch_gather(data, seed, step, True, B, out=obs_b)
    hip.gemm_grouped([dict(A=obs_b, B=w, out=out_b)])
    torch.cuda.synchronize()
    assert_bits(obs.cpu(), rows, "1000 tiles: obs"); assert_bits(obs_b.cpu(), rows, "1000 tiles: obs of air_batch_gather")
    assert_close(out, rows.double() @ w.double().cpu(), *FC.product_tol(K), f"product {B}x{N}x{K}", "I")
    assert_bits(buf, buf_b, "1000 tiles: product against air_batch_gather + air_gemm_grouped")


def test_gather_declines_a_group_air_gemm_grouped_runs_on_the_wide_tile_kernels(hip):
    """One column of tiles more: air_gemm_grouped tests its wide-tile regime (more than wide_min_tiles() tiles, aligned operands, N and
    K multiples of 4) BEFORE the long-K split and runs this product on gemm_wide_kernel, the gather would run it on 16 waves.  The
    rule took such groups up to 1024 tiles; it now stops at wide_min_tiles(), and the engine plans the two launches."""
    B, N, K = FC.GG_EDGE_DECLINED
    data, w, seed, step, obs, buf, out, bg, rows = _lone_gather(hip, B, N, K)
    probs = [dict(A=obs, B=w, out=out)]
    assert hip.gemm_grouped_gather_fits(probs, bg) == 0
    st, _ = hip.gemm_grouped_gather(probs, bg)
    torch.cuda.synchronize()
    assert st == hip.E_UNSUPPORTED and bool((obs == SENTINEL).all()) and bool(torch.isnan(out).all())
    hip.batch_gather(data, seed, step, True, B, out=obs)
    hip.gemm_grouped(probs)
    torch.cuda.synchronize()
    assert_bits(obs.cpu(), rows, "1004 tiles: obs")
    assert_close(out, rows.double() @ w.double().cpu(), *FC.product_tol(K), f"product {B}x{N}x{K}", "I")
    assert_padding(buf, N, "1004 tiles: product")


# ---------------------------------------------------------------------------------------------------------------
# J. the step prologue and the first LSTM step
# ---------------------------------------------------------------------------------------------------------------
def _noise_buffers(n_normal, n_uniform):
    nb = torch.full((n_normal + 1,), SENTINEL, dtype=torch.float32, device="cuda"); nb[:n_normal] = NAN
    ub = torch.full((n_uniform + 1,), SENTINEL, dtype=torch.float32, device="cuda"); ub[:n_uniform] = NAN
    return nb, ub, (nb[:n_normal] if n_normal else None), (ub[:n_uniform] if n_uniform else None)


@pytest.fixture(scope="module")
def noise_refs():
    return {sz: FC.noise_ref(FC.RNG_SEED, FC.RNG_OFFSET, *sz) for sz in FC.NOISE_SIZES}


def _check_noise(nb, ub, sizes, refs, tag):
    n_normal, n_uniform = sizes
    z64, u32 = refs[sizes]
    assert_bits(ub[:n_uniform].cpu(), u32, tag + "uniforms")
    assert_close(nb[:n_normal], z64, *FC.NORMAL_TOL, tag + "normals", "J")
    assert float(nb[n_normal]) == SENTINEL and float(ub[n_uniform]) == SENTINEL, tag + "the element behind the end"


def _check_tiles(h_t, c_t, h0, c0, B, tag):
    assert_bits(h_t.cpu(), h0[None, :].expand(B, -1).contiguous(), tag + "h_tiled")
    assert_bits(c_t.cpu(), c0[None, :].expand(B, -1).contiguous(), tag + "c_tiled")


SCHED = dict(init=0.9, final_value=1e-3, anneal_type="exp", anneal_steps=1000.0, hold_for=100.0, steps_div=10.0)
GSTEP, T_PRIOR = 600, 5


def _prior_ref():
    return FC.prior_ref("exp", 0.9, 1e-3, 1000.0, 100.0, 10.0, GSTEP, T_PRIOR)


@pytest.mark.parametrize("sizes,shape", list(zip(FC.NOISE_SIZES, [(5, 7), (37, 50), (1045, 128), (5, 7)])))
def test_step_prologue_noise_prior_and_tiled_state(hip, noise_refs, sizes, shape):
    B, Hd = shape
    tag = f"prologue {sizes} {shape} "
    gen = torch.Generator().manual_seed(B)
    h0, c0 = torch.randn(Hd, generator=gen), torch.randn(Hd, generator=gen)
    rng, gstep = i64(FC.RNG_SEED, FC.RNG_OFFSET), i64(GSTEP)
    nb, ub, normal, uniform = _noise_buffers(*sizes)
    prior, h_t, c_t, _ = hip.step_prologue(normal, uniform, rng, gstep, T_PRIOR, g(h0), g(c0), B, **SCHED)
    torch.cuda.synchronize()
    _check_noise(nb, ub, sizes, noise_refs, tag)
    assert_close(prior, _prior_ref(), *FC.PRIOR_TOL, tag + "prior", "J")
    _check_tiles(h_t, c_t, h0, c0, B, tag)
    assert rng.tolist() == [FC.RNG_SEED, FC.RNG_OFFSET] and gstep.tolist() == [GSTEP]          # the prologue advances nothing


def test_step_prologue_prior_schedules(hip):
    h0 = torch.zeros(7).cuda()
    for anneal, init, final, steps, hold, div, gsteps in FC.PRIOR_SCHEDULES:
        for s in gsteps:
            rng, gstep = i64(1, 0), i64(s)
            for T in (1, 5):
                prior, _, _, _ = hip.step_prologue(None, None, rng, gstep, T, h0, h0, 5, init, final, anneal, steps, hold, div)
                assert_close(prior, FC.prior_ref(anneal, init, final, steps, hold, div, s, T), *FC.PRIOR_TOL,
                             f"prologue prior {anneal} step {s} T {T}", "J")


def test_step_prologue_cvt_and_gather_cvt(hip, noise_refs):
    sizes, B, Hd, n = (4097, 4099), 37, 50, 2500
    gen = torch.Generator().manual_seed(12)
    h0, c0 = torch.randn(Hd, generator=gen), torch.randn(Hd, generator=gen)
    data = torch.randn(41, n, generator=gen)
    idx = FC.feeder_indices(FC.FEED_SEED, 3, B, 41, True)
    rows = data[torch.tensor(idx)]
    rng, gstep = i64(FC.RNG_SEED, FC.RNG_OFFSET), i64(GSTEP)
    # _cvt: the mirror of a batch given in place
    nb, ub, normal, uniform = _noise_buffers(*sizes)
    prior, h_t, c_t, x16 = hip.step_prologue(normal, uniform, rng, gstep, T_PRIOR, g(h0), g(c0), B, x=g(rows), **SCHED)
    torch.cuda.synchronize()
    _check_noise(nb, ub, sizes, noise_refs, "prologue_cvt ")
    assert_close(prior, _prior_ref(), *FC.PRIOR_TOL, "prologue_cvt prior", "J"); _check_tiles(h_t, c_t, h0, c0, B, "prologue_cvt ")
    assert torch.equal(x16.cpu().view(torch.int16), rows.to(torch.bfloat16).view(torch.int16)), "prologue_cvt: the bf16 mirror"
    # _gather_cvt: the rows drawn from the dataset, written to obs and to the mirror
    nb, ub, normal, uniform = _noise_buffers(*sizes)
    obs_buf = torch.full((B * n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    obs = obs_buf[:B * n].view(B, n); obs.fill_(NAN)
    idx_out = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    data_d, seed, step = g(data), i64(FC.FEED_SEED), i64(3)
    bg = hip.batch_gather_desc(data_d, seed, step, True, obs, idx_out)
    prior, h_t, c_t, x16 = hip.step_prologue(normal, uniform, rng, gstep, T_PRIOR, g(h0), g(c0), B, gather=bg, **SCHED)
    torch.cuda.synchronize()
    _check_noise(nb, ub, sizes, noise_refs, "prologue_gather_cvt ")
    assert_close(prior, _prior_ref(), *FC.PRIOR_TOL, "prologue_gather_cvt prior", "J"); _check_tiles(h_t, c_t, h0, c0, B, "prologue_gather_cvt ")
    assert idx_out.tolist() == idx
    assert_bits(obs.cpu(), rows, "prologue_gather_cvt: obs"); assert bool((obs_buf[B * n:] == SENTINEL).all())
    assert torch.equal(x16.cpu().view(torch.int16), rows.to(torch.bfloat16).view(torch.int16)), "prologue_gather_cvt: the bf16 mirror"


NOISE_J = (4097, 4099)


@pytest.mark.parametrize("precision", [FC.F32, FC.BF16])
@pytest.mark.parametrize("M,Hd", FC.LSTM_PRO_SHAPES)
def test_lstm_step_fwd_prologue(hip, noise_refs, M, Hd, precision):
    c = FC.lstm_case(M, Hd)
    tag = f"lstm_step_fwd_prologue {M}x{Hd} prec={precision} "
    h0, c0, w_h, gx = g(c["h0"]), g(c["c0"]), g(c["w_h"]), g(c["gx"])
    rng, gstep = i64(FC.RNG_SEED, FC.RNG_OFFSET), i64(GSTEP)
    nb, ub, normal, uniform = _noise_buffers(*NOISE_J)
    (h, cc, act), (prior, h_t, c_t) = hip.lstm_step_fwd_prologue(h0, c0, w_h, gx, 1.0, precision, normal, uniform, rng, gstep, T_PRIOR, **SCHED)
    # the two launches it replaces
    nb2, ub2, normal2, uniform2 = _noise_buffers(*NOISE_J)
    prior2, h_t2, c_t2, _ = hip.step_prologue(normal2, uniform2, rng, gstep, T_PRIOR, h0, c0, M, **SCHED)
    h2, cc2, act2 = hip.lstm_step_fwd(h_t2, c_t2, w_h, gx, 1.0, precision)
    torch.cuda.synchronize()
    _, h64, c64, act64 = FC.lstm_refs(c, precision)
    assert_close(h, h64, *FC.LSTM_TOL, tag + "h", "J"); assert_close(cc, c64, *FC.LSTM_TOL, tag + "c", "J")
    assert_close(act, act64, *FC.LSTM_TOL, tag + "gate_act", "J")
    _check_noise(nb, ub, NOISE_J, noise_refs, tag)
    assert_close(prior, _prior_ref(), *FC.PRIOR_TOL, tag + "prior", "J")
    _check_tiles(h_t, c_t, c["h0"], c["c0"], M, tag)
    for a, b, nm in ((h, h2, "h"), (cc, cc2, "c"), (act, act2, "gate_act"), (nb, nb2, "normals"), (ub, ub2, "uniforms"), (h_t, h_t2, "h_tiled"),
                     (c_t, c_t2, "c_tiled")):
        assert_bits(a, b, tag + nm + " against air_step_prologue + air_lstm_step_fwd")
    assert torch.equal(prior, prior2)


def _first_inputs(c, shifted):
    M, Hd, E, ldx = c["M"], c["Hd"], c["E"], c["ldx"]
    flat = torch.zeros(M * ldx + 4, dtype=torch.float32, device="cuda")
    o = 1 if shifted else 0
    xb = flat[o:o + M * ldx].view(M, ldx)
    xb.copy_(g(c["x_buf"]))
    wf = g(c["w_full"])
    return xb[:, :E], wf[:E], wf[E:], g(c["b"]), g(c["h0"]), g(c["c0"])


@pytest.mark.parametrize("precision", [FC.F32, FC.BF16])
@pytest.mark.parametrize("i", range(len(FC.FIRST_CASES)))
def test_lstm_first_step_fwd(hip, noise_refs, i, precision):
    M, Hd, E, ldx, shifted = FC.FIRST_CASES[i]
    c = FC.lstm_case(M, Hd, E, ldx)
    tag = f"lstm_first_step_fwd case {i} prec={precision} "
    x, w_x, w_h, b, h0, c0 = _first_inputs(c, shifted)
    assert (x.data_ptr() % 16 == 0) == (not shifted)
    rng, gstep = i64(FC.RNG_SEED, FC.RNG_OFFSET), i64(GSTEP)
    nb, ub, normal, uniform = _noise_buffers(*NOISE_J)
    gbuf, gx = padded(M, 4 * Hd, 4 * Hd + 4)
    st, (h, cc, act), (prior, h_t, c_t) = hip.lstm_first_step_fwd(x, w_x, b, h0, c0, w_h, gx, 1.0, precision, normal, uniform, rng, gstep,
                                                                   T_PRIOR, **SCHED)
    assert st == 0
    # the two launches it replaces: the gx product with its bias, then the first step with the prologue
    nb2, ub2, normal2, uniform2 = _noise_buffers(*NOISE_J)
    gbuf2, gx2 = padded(M, 4 * Hd, 4 * Hd + 4)
    hip.gemm_grouped([dict(A=x, B=w_x, bias=b, epilogue=hip.EPI_BIAS, out=gx2)], precision=precision)
    (h2, cc2, act2), (prior2, h_t2, c_t2) = hip.lstm_step_fwd_prologue(h0, c0, w_h, gx2, 1.0, precision, normal2, uniform2, rng, gstep, T_PRIOR,
                                                                        **SCHED)
    torch.cuda.synchronize()
    gx64, _, _, _ = FC.lstm_refs(c, precision)
    assert_close(gx, gx64, *FC.product_tol(E), tag + "gx_out", "J")
    assert_padding(gbuf, 4 * Hd, tag + "gx_out")
    h64, c64, act64 = FC.lstm64(c["h0"][None, :], c["c0"][None, :], c["w_h"], gx.cpu(), 1.0, precision)       # on the gx the launch wrote
    assert_close(h, h64, *FC.LSTM_TOL, tag + "h", "J"); assert_close(cc, c64, *FC.LSTM_TOL, tag + "c", "J")
    assert_close(act, act64, *FC.LSTM_TOL, tag + "gate_act", "J")
    _check_noise(nb, ub, NOISE_J, noise_refs, tag)
    assert_close(prior, _prior_ref(), *FC.PRIOR_TOL, tag + "prior", "J")
    _check_tiles(h_t, c_t, c["h0"], c["c0"], M, tag)
    for a, bb, nm in ((gbuf, gbuf2, "gx_out"), (h, h2, "h"), (cc, cc2, "c"), (act, act2, "gate_act"), (nb, nb2, "normals"), (ub, ub2, "uniforms"),
                      (h_t, h_t2, "h_tiled"), (c_t, c_t2, "c_tiled")):
        assert_bits(a, bb, tag + nm + " against the gx product + air_lstm_step_fwd_prologue")
    assert torch.equal(prior, prior2)


@pytest.mark.parametrize("why", sorted(FC.FIRST_DECLINED))
def test_lstm_first_step_fwd_declines(hip, why):
    """beyond 512 tiles of (M, Hd), and wherever air_gemm_grouped would run the gx product on another body than the 4-wave 16 x 16 one
    whose K order the launch repeats: there its results would not be those of the two launches it replaces (at M = 512, Hd = 256,
    E = 52 with bf16 operands 22 358 of the 526 336 elements of gx differed before the launch declined the shape)"""
    M, Hd, E, ldx = FC.FIRST_DECLINED[why]
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    gx = nans(M, 4 * Hd)
    wf = z(E + Hd, 4 * Hd)
    for precision in (FC.F32, FC.BF16):
        st, (h, cc, act), (prior, h_t, c_t) = hip.lstm_first_step_fwd(z(M, ldx)[:, :E], wf[:E], z(4 * Hd), z(Hd), z(Hd), wf[E:], gx, 1.0, precision,
                                                                       None, None, i64(1, 0), i64(0), T_PRIOR, 0.3)
        torch.cuda.synchronize()
        assert st == hip.E_UNSUPPORTED, why
        assert all(bool(torch.isnan(t).all()) for t in (gx, h, cc, act, prior, h_t, c_t)), why


# ---------------------------------------------------------------------------------------------------------------
# K. the small riders
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(FC.CANVAS_SHAPES)))
def test_canvas_unroll_bwd_dpresence_and_nvil(hip, i):
    c = FC.canvas_case(i)
    T, B = c["T"], c["B"]
    tag = f"canvas case {i} "
    glm, where, pres, obs = g(c["glimpse"]), g(c["where"]), g(c["presence"]), g(c["obs"])
    mult, std, ls = FC.CANVAS_MULT, FC.CANVAS_STD, c["loss_scale"]
    _, final, _ = hip.canvas_unroll_fwd(glm, where, pres, (c["H"], c["W"]), obs=obs, mult=mult, std=std, keep_steps=False)
    for fc, form in ((final, "stored canvas"), (None, "recomputed canvas")):
        dg0, dw0 = hip.canvas_unroll_bwd(glm, where, pres, obs, fc, mult, std, ls)
        dg, dw, dpres = hip.canvas_unroll_bwd_dpresence(glm, where, pres, obs, fc, mult, std, ls)
        torch.cuda.synchronize()
        ref = c["dpresence64"]
        scale = ref.abs() + 1.0
        assert_close(dpres.cpu().double() / scale, ref / scale, *FC.DPRESENCE_TOL, tag + form + " dpresence", "K")
        assert_bits(dg, dg0, tag + form + " dglimpse against air_canvas_unroll_bwd")
        assert_bits(dw, dw0, tag + form + " dwhere against air_canvas_unroll_bwd")
    dg0, dw0 = hip.canvas_unroll_bwd(glm, where, pres, obs, final, mult, std, ls)
    gen = torch.Generator().manual_seed(31 + i)
    base = (torch.randn(B, generator=gen) * 10).cuda(); logp = (-torch.rand(B, generator=gen) * 3).cuda()
    for n_parts in (1, 4):
        parts = (torch.rand(n_parts, B, generator=gen) * torch.tensor([2000.0, 300.0, 40.0, 5.0])[:n_parts, None] + 7.0).cuda()
        for with_ema in (False, True):
            ema_a = torch.tensor([800.0, 9.0, 0.9, 1.0]).cuda() if with_ema else None
            ema_b = ema_a.clone() if with_ema else None
            dg, dw, (out, dlogp, dbase, imp_sum) = hip.canvas_unroll_bwd_nvil(glm, where, pres, obs, final, mult, std, ls, parts, base, logp, ema_a)
            rout, rdlogp, rdbase, rsum = hip.nvil_parts(parts, base, logp, ema_b)
            torch.cuda.synchronize()
            t2 = tag + f"n_parts={n_parts} ema={with_ema} "
            assert_bits(dg, dg0, t2 + "dglimpse"); assert_bits(dw, dw0, t2 + "dwhere")
            assert_bits(out, rout, t2 + "nvil out"); assert_bits(dlogp, rdlogp, t2 + "dlogp"); assert_bits(dbase, rdbase, t2 + "dbaseline")
            assert_bits(imp_sum, rsum, t2 + "imp_sum")
            assert bool(torch.isfinite(out).all())
            if with_ema:
                assert_bits(ema_a, ema_b, t2 + "moving averages")


@pytest.mark.parametrize("T,n", FC.SUM_LEADING)
def test_sum_leading(hip, T, n):
    x = torch.randn(T, n, generator=torch.Generator().manual_seed(T * 10000 + n))
    out = hip.sum_leading(x.cuda())
    torch.cuda.synchronize()
    assert_bits(out.cpu(), FC.sum_in_order32(x), f"sum_leading T={T} n={n}: the float32 sum in order from part 0")
    # T - 1 roundings (0 + x_0 is exact), each at most half an ulp of a partial sum that is at most sum |x_t|
    bound = (T - 1) * 2.0 ** -24 * x.double().abs().sum(0)
    assert bool(((out.cpu().double() - x.double().sum(0)).abs() <= bound).all())


def test_l2_grad_add_and_counter_add(hip):
    gen = torch.Generator().manual_seed(8)
    n, l2 = 1000, 1e-3
    g0, p0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ranges = [(4, 300), (300, 300), (513, 777)]
    gd = g0.cuda()
    hip.l2_grad_add_(gd, p0.cuda(), ranges, l2)
    torch.cuda.synchronize()
    t = torch.zeros(n, dtype=torch.bool)
    for lo, hi in ranges:
        t[lo:hi] = True
    ref = g0.double() + FC.f32v(l2) * p0.double()                   # g += l2_weight * p
    assert_close(gd.cpu()[t], ref[t], 2.0 ** -23, 1e-9, "l2_grad_add", "K")        # one float32 rounding, fused or not
    assert_bits(gd.cpu()[~t], g0[~t], "l2_grad_add outside the ranges")
    counter = i64(5, 77, -1)
    hip.counter_add_(counter, 2 ** 40 + 3)
    hip.counter_add_(counter, -1)
    torch.cuda.synchronize()
    assert counter.tolist() == [5 + 2 ** 40 + 2, 77, -1]
