"""GPU parity of the Gaussian nodes, the optimiser, the bf16 casts and the utilities, one launch at a time through the C ABI (run with
-m gpu on an MI355X).  Cases, references, restatements and bounds come from tests/pointwise_cases.py; tests/test_pointwise_cases_host.py
holds them on the CPU.

Per case: every operand is a window of a NaN-filled parent, every output a NaN-primed window of a SENTINEL-filled parent (the gaps of
ld_dpre = 2D + 5 hold the SENTINEL too), every in-place buffer a window of a SENTINEL parent; after the launch the status is 0, every
output element is written, and every parent is unchanged to the bit outside what the launch owns.  A refused call returns its status
and writes nothing.
  Ga  loc (loc_mode 0: bits of pre), scale, sample, kl_row, dpre, dloc / dscale within CONST * 2^-24 * S of float64 autograd; a floored
      scale is the guard's bits, its gradient and a saturated sigmoid' / tanh' exactly 0; air_normal_kl_fwd on the written loc / scale:
      the bits of the forward's kl_row; air_gauss_sample_bwd_nvil at 8197 x 65: dpre the bits of air_gauss_sample_bwd with and without
      KL shares, the NVIL outputs those of air_nvil_parts, kl_row_out those of fold_cases.sum_in_order32; air_heads_fwd / _bwd at
      (T, B) = (32, 257), (8, 1025), (9, 1025): every output the bits of the stand-alone launches.
  Op  the centred update in every carrier (air_rmsprop, air_rmsprop_centered, both forms of air_step_epilogue / _shadow, the rider of
      air_lstm_pointwise_bwd_opt): the BITS of the float32 restatement rmsprop32 in p, ms, mg and mom, NaN positions included; the
      carriers against each other bit for bit; the plain update within fold_cases.RMS_TOL of float64; the counters; air_l2_grad_add.
  Bf  bits of the integer round-to-nearest-even; a NaN stays a NaN.
  Ut  air_fill, air_tile_rows: bits; air_axpby: 2^-23 relative; air_colsum: the bits of the ordered float32 sum.
The worst error / bound of each group is printed when the module finishes (pytest -s).

Worst error / bound on an MI355X (the float32 restatement on the CPU: 0.246 / 0.246 / 0.212 / 0.179 / 0.237 / 0.239 of the bound): Ga
loc 0.246 (Ga_8197x4_where), scale 0.252 (Ga_8197x65), sample 0.203 (Ga_8197x4_where), kl_row 0.233 (Ga_guard_where), dpre 0.237
(Ga_41x50_no_kl [no_dkl]), air_normal_kl_bwd 0.239 (dscale of Ga_8197x65); Op 0.497 (L2_strided against the one-rounding bar; the plain
update against RMS_TOL below it); Ut 0.992 (colsum 3 x 524291 against (M - 1) 2^-24 sum|x|; its bits are the ordered float32 sum's).
Every bit bar holds: all carriers of the centred update give the restatement's bits in every case, NaN positions included -- the
device's float32 division and square root round as IEEE's, no launch had to fall back to RMS_TOL; every cast is the integer
round-to-nearest-even, no subnormal flushed, every NaN kept.  No kernel and no launch rule had to change."""
import ctypes

import numpy as np
import pytest
import torch

import attend_cases as AC
import fold_cases as FC
import pointwise_cases as PC
from attend_cases import SENTINEL, assert_close, print_worst
from oracle import air_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print_worst("pointwise kernels", ["Ga", "Op", "Ut"])


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Stage:
    """the operands of one launch on the device, and the check of everything the launch must not have touched"""

    def __init__(self):
        self.items = []                                         # (name, win, device parent, device view, kind)

    def _add(self, name, win, kind):
        par, v = win.cuda()
        self.items.append((name, win, par, v, kind))
        return v

    def inp(self, name, values, off=False):
        """an operand: values [..] as a window of a NaN parent (NaN entries of `values` stay what they are)"""
        v = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.float32)
        win = PC.Win(v.shape, off)
        win.v.copy_(v)
        return self._add(name, win, "in")

    def inp_bits(self, name, u32, off=False):
        win = PC.Win((len(u32),), off)
        win.v.view(torch.int32).copy_(torch.from_numpy(np.ascontiguousarray(u32).view(np.int32)))
        return self._add(name, win, "in")

    def out(self, name, shape, off=False, gap_from=None):
        """an output: NaN-primed window of a SENTINEL parent; gap_from: the columns from there on are no part of the output (SENTINEL)"""
        win = PC.out_win(shape, off)
        if gap_from is not None:
            win.v[:, gap_from:] = SENTINEL
        return self._add(name, win, ("out", gap_from))

    def state(self, name, values, off=False):
        return self._add(name, PC.state_win(values, off), "state")

    def out16(self, name, n, off=False):
        win = PC.Win16(n, off)
        par, v = win.cuda()
        self.items.append((name, win, par, v, "out16"))
        return v

    def untouched(self, written=True):
        """inputs: the whole parent keeps its bits; outputs / state: the SENTINEL around the window (and in the gap columns) keeps its
        bits; written = False (a refused call): every output still holds its primer, every state its values"""
        torch.cuda.synchronize()
        for name, win, par, v, kind in self.items:
            if kind == "out16":
                assert win.intact(par), f"{name}: written outside its window"
                if not written:
                    assert bool((v.cpu() == win.parent[win.lead:win.lead + win.n]).all()), f"{name}: written by a refused call"
                continue
            if kind == "in" or (not written):
                same = bits(par) == win.parent.view(torch.int32)
                assert bool(same.all()), f"{name}: {int((~same).sum())} elements of an operand the launch must not write have changed"
                continue
            assert PC.surroundings_intact(win, par), f"{name}: written outside its window"
            if isinstance(kind, tuple) and kind[1] is not None:
                gap = v[:, kind[1]:]
                assert bool((bits(gap) == torch.full(tuple(gap.shape), SENTINEL).view(torch.int32)).all()), f"{name}: the gap columns were written"


def within(out, ref64, S, kind, what):
    """|out - ref64| <= PC.ga_bound(kind, S) elementwise (S == 0: exactly equal); the worst ratio goes to the report of group Ga"""
    out = out.detach().cpu().double().numpy() if torch.is_tensor(out) else np.asarray(out, np.float64)
    ref64, S = np.asarray(ref64, np.float64), np.asarray(S, np.float64)
    assert out.shape == ref64.shape == S.shape, f"{what}: {out.shape} {ref64.shape} {S.shape}"
    assert np.isfinite(out).all(), f"{what}: {int((~np.isfinite(out)).sum())} elements not finite (an output left unwritten?)"
    err = np.abs(out - ref64)
    assert (err[S == 0] == 0).all(), f"{what}: differs where the bound is zero"
    nz = S > 0
    if nz.any():
        ratio = err[nz] / PC.ga_bound(kind, S[nz])
        worst = float(ratio.max())
        print(f"\n  {what}: worst error / bound {worst:.3g}")
        if "Ga" not in AC.WORST or worst > AC.WORST["Ga"][0]:
            AC.WORST["Ga"] = (worst, what)
        assert worst <= 1.0, f"{what}: worst error / bound {worst:.3g}"


def same(a, b, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    n = PC.same_bits_or_nan(a, b)
    assert n == 0, f"{what}: {n} of {a.size} elements differ in their bits (or in where the NaNs fall)"


# ---------------------------------------------------------------------------------------------------------------
# Ga
# ---------------------------------------------------------------------------------------------------------------
def _pre_wide(d):
    c = d["case"]
    wide = np.full((c["M"], c["ld_pre"]), np.nan, F32)
    wide[:, :2 * c["D"]] = d["pre"]
    return wide


def _fwd_launch(hip, st, d, c, pre, eps, loc, scale, sample, kl, ld_pre=None, loc_mode=None, M=None):
    return hip.lib().air_gauss_sample_fwd(P(pre), c["ld_pre"] if ld_pre is None else ld_pre, P(eps), c["offset"],
                                          c["loc_mode"] if loc_mode is None else loc_mode, *c["prior4"], P(loc), P(scale), P(sample), P(kl),
                                          c["M"] if M is None else M, c["D"], c["guard"], stream())


@pytest.mark.parametrize("name", PC.GA_RUN)
def test_Ga_gauss_sample_fwd_and_normal_kl_fwd(hip, name):
    d, c = PC.ga_data(name), PC.GA[name]
    M, D = c["M"], c["D"]
    f = PC.ga_fwd_ref(name)
    t = f["terms"]
    st = Stage()
    pre = st.inp("pre", _pre_wide(d))
    eps = st.inp("eps", d["eps"]) if c["fwd"] != "no_sample" else None
    loc, scale = st.out("loc", (M, D)), st.out("scale", (M, D))
    sample = st.out("sample", (M, D)) if c["fwd"] != "no_sample" else None
    kl = st.out("kl_row", (M,)) if c["fwd"] != "no_kl" else None
    assert _fwd_launch(hip, st, d, c, pre, eps, loc, scale, sample, kl) == 0
    st.untouched()
    if c["loc_mode"] == 0:
        same(loc, d["pre"][:, :D], f"{name} loc (a copy of pre)")
    else:
        within(loc, f["loc"], t["S_loc"], "loc", f"{name} loc")
    within(scale, f["scale"], t["S_scale"], "scale", f"{name} scale")
    for r_, dd in d["planted"].get("floored", []) + (d["planted"].get("small", []) if c["guard"] > 0 else []):
        assert scale[r_, dd].item() == FC.f32v(PC.GUARD), f"{name}: a floored scale is the guard"
    if sample is not None:
        within(sample, f["sample"], t["S_sample"], "sample", f"{name} sample")
        G = FC.f32v(PC.GUARD)
        for (r_, dd), want in zip(d["planted"].get("where_floor", []), (G, G, G, -G)):
            assert sample[r_, dd].item() == want, f"{name}: the floored where-scale sample at {(r_, dd)}"
    if kl is not None:
        within(kl, f["kl_row"], t["S_kl_row"], "kl_row", f"{name} kl_row")
    # air_normal_kl_fwd on the loc / scale just written
    st2 = Stage()
    loc_in, scale_in = st2.inp("loc", loc.cpu().numpy()), st2.inp("scale", scale.cpu().numpy())
    kl2 = st2.out("kl_row", (M,))
    assert hip.lib().air_normal_kl_fwd(P(loc_in), P(scale_in), *c["prior4"], P(kl2), M, D, stream()) == 0
    st2.untouched()
    if kl is not None:
        same(kl2, kl, f"{name} air_normal_kl_fwd against the forward's kl_row")
    else:
        within(kl2, f["kl_row"], t["S_kl_row"], "kl_row", f"{name} air_normal_kl_fwd")


def _bwd_args(st, d, c, opt, scale32=None):
    kw = PC.ga_bwd_inputs(d, opt)
    M, D = c["M"], c["D"]
    a = dict(pre=st.inp("pre", _pre_wide(d)), eps=None if kw["eps"] is None else st.inp("eps", kw["eps"]),
             loc=st.inp("loc", d["loc32"]), scale=st.inp("scale", d["scale32"] if scale32 is None else scale32),
             dsample=None if kw["dsample"] is None else st.inp("dsample", kw["dsample"]),
             dsample2=None if kw["dsample2"] is None else st.inp("dsample2", kw["dsample2"]),
             dkl_row=None if kw["dkl_row"] is None else st.inp("dkl_row", kw["dkl_row"]), dkl_scale=kw["dkl_scale"],
             dpre=st.out("dpre", (M, c["ld_dpre"]), gap_from=2 * D))
    return a


def _bwd_head(c, a, ld_pre=None, ld_dpre=None, M=None):
    return (P(a["pre"]), c["ld_pre"] if ld_pre is None else ld_pre, P(a["eps"]), c["offset"], c["loc_mode"], *c["prior4"], P(a["loc"]),
            P(a["scale"]), P(a["dsample"]), P(a["dsample2"]), P(a["dkl_row"]), a["dkl_scale"], P(a["dpre"]),
            c["ld_dpre"] if ld_dpre is None else ld_dpre, c["M"] if M is None else M, c["D"])


@pytest.mark.parametrize("name,opt", [(n, o) for n in PC.GA_RUN for o in PC.GA[n]["bwd"]])
def test_Ga_gauss_sample_bwd(hip, name, opt):
    d, c = PC.ga_data(name), PC.GA[name]
    D = c["D"]
    ref, S, _ = PC.ga_bwd_ref(name, opt)
    st = Stage()
    a = _bwd_args(st, d, c, opt)
    assert hip.lib().air_gauss_sample_bwd(*_bwd_head(c, a), c["guard"], None, 0, None, stream()) == 0
    st.untouched()
    dpre = a["dpre"][:, :2 * D]
    within(dpre, ref, S, "dpre", f"{name} [{opt}] dpre")
    for (r_, dd), zero in zip(d["planted"].get("saturated", []), (True, True, False, True)):
        if zero:
            assert dpre[r_, dd].item() == 0.0, f"{name}: the derivative factor of a saturated loc is exactly 0"
    if c["guard"] > 0:
        for r_, dd in d["planted"].get("floored", []) + d["planted"].get("small", []):
            assert dpre[r_, D + dd].item() == 0.0, f"{name}: a floored scale passes no gradient"


def test_Ga_stored_scale_at_under_and_over_the_guard(hip):
    """`s <= guard` of gauss_bwd_elem on the stored scale: exactly the guard and the float32 under it pass no gradient, the float32 over it
    passes the gradient of the head written out at that scale"""
    name, opt = "Ga_guard_41x50", "ds_ds2"
    d, c = PC.ga_data(name), PC.GA[name]
    D = c["D"]
    kw = PC.ga_bwd_inputs(d, opt)
    scale = d["scale32"].copy()
    spots = [(20, 7), (21, 8), (22, 9)]
    for (r_, dd), (s, _) in zip(spots, PC.guard_scales()):
        scale[r_, dd] = s
    t = PC.gauss_terms64(d["pre"], kw["eps"], D, c["loc_mode"], c["offset"], c["prior4"], loc=d["loc32"], scale=scale, dsample=kw["dsample"],
                         dsample2=kw["dsample2"], dkl_row=kw["dkl_row"], dkl_scale=kw["dkl_scale"], guard=c["guard"])
    st = Stage()
    a = _bwd_args(st, d, c, opt, scale32=scale)
    assert hip.lib().air_gauss_sample_bwd(*_bwd_head(c, a), c["guard"], None, 0, None, stream()) == 0
    st.untouched()
    dpre = a["dpre"][:, :2 * D].cpu().numpy()
    for (r_, dd), (s, passes) in zip(spots, PC.guard_scales()):
        if passes:
            assert dpre[r_, D + dd] != 0.0
            within(dpre[r_:r_ + 1, D + dd:D + dd + 1], t["dpre"][r_:r_ + 1, D + dd:D + dd + 1], t["S_dpre"][r_:r_ + 1, D + dd:D + dd + 1],
                   "dpre", "the stored scale one float32 over the guard")
        else:
            assert dpre[r_, D + dd] == 0.0 and t["dpre"][r_, D + dd] == 0.0, (r_, dd, float(s))


@pytest.mark.parametrize("name", [n for n in PC.GA_RUN if PC.GA[n]["kl_bwd"]])
def test_Ga_normal_kl_bwd(hip, name):
    d, c = PC.ga_data(name), PC.GA[name]
    M, D = c["M"], c["D"]
    dl, dsc, S_l, S_s = PC.normal_kl_bwd64(d["loc32"], d["scale32"], c["prior4"], d["dkl_row"])
    st = Stage()
    loc, scale, dkl = st.inp("loc", d["loc32"]), st.inp("scale", d["scale32"]), st.inp("dkl_row", d["dkl_row"])
    dloc, dscale = st.out("dloc", (M, D)), st.out("dscale", (M, D))
    assert hip.lib().air_normal_kl_bwd(P(loc), P(scale), *c["prior4"], P(dkl), P(dloc), P(dscale), M, D, stream()) == 0
    st.untouched()
    within(dloc, dl, S_l, "kl_bwd", f"{name} normal_kl_bwd dloc")
    within(dscale, dsc, S_s, "kl_bwd", f"{name} normal_kl_bwd dscale")


def test_Ga_gauss_sample_bwd_nvil_equals_its_parts_bit_for_bit(hip):
    """at 8197 x 65 the Gaussian part of the grid sits at its cap (532 805 items): air_gauss_sample_bwd_nvil's virtual block index
    (blockIdx.x - 1 of gridDim.x - 1, or - 2 with the KL-share workgroup behind) and air_gauss_sample_bwd's with the share workgroup"""
    name, opt = "Ga_8197x65", "ds_ds2"
    d, c = PC.ga_data(name), PC.GA[name]
    M, D = c["M"], c["D"]
    assert M * D > PC.CAP_ITEMS
    nv = PC.nvil_inputs(M=M)
    B, n_parts, n_kl = nv["baseline"].shape[0], nv["imp_parts"].shape[0], nv["kl_parts"].shape[0]
    lib = hip.lib()
    results = []
    for with_nvil in (False, True):
        for shares in (0, n_kl):
            st = Stage()
            a = _bwd_args(st, d, c, opt)
            klp = st.inp("kl_parts", nv["kl_parts"]) if shares else None
            klo = st.out("kl_row_out", (M,)) if shares else None
            r = dict(dpre=a["dpre"], kl_row_out=klo)
            if with_nvil:
                imp, base, logp = st.inp("imp_parts", nv["imp_parts"]), st.inp("baseline", nv["baseline"]), st.inp("logp", nv["logp"])
                ema = st.state("ema", nv["ema"])
                r.update(out=st.out("nvil_out", (4,)), dlogp=st.out("dlogp", (B,)), dbase=st.out("dbaseline", (B,)),
                         imp_sum=st.out("imp_sum", (B,)), ema=ema)
                status = lib.air_gauss_sample_bwd_nvil(*_bwd_head(c, a), P(imp), n_parts, P(r["imp_sum"]), P(base), P(logp), P(r["out"]),
                                                       P(r["dlogp"]), P(r["dbase"]), B, c["guard"], P(ema), P(klp), shares, P(klo), stream())
            else:
                status = lib.air_gauss_sample_bwd(*_bwd_head(c, a), c["guard"], P(klp), shares, P(klo), stream())
            assert status == 0
            st.untouched()
            results.append(r)
    for r in results[1:]:
        same(r["dpre"], results[0]["dpre"], "dpre of the launch with riders against air_gauss_sample_bwd alone")
    for r in (results[1], results[3]):
        same(r["kl_row_out"], FC.sum_in_order32(torch.from_numpy(nv["kl_parts"])), "kl_row_out against the shares added in order")
    st = Stage()
    imp, base, logp = st.inp("imp_parts", nv["imp_parts"]), st.inp("baseline", nv["baseline"]), st.inp("logp", nv["logp"])
    ema = st.state("ema", nv["ema"])
    out, dlogp, dbase, imp_sum = st.out("nvil_out", (4,)), st.out("dlogp", (B,)), st.out("dbaseline", (B,)), st.out("imp_sum", (B,))
    assert lib.air_nvil_parts(P(imp), n_parts, P(imp_sum), P(base), P(logp), P(out), P(dlogp), P(dbase), B, P(ema), stream()) == 0
    st.untouched()
    for r in (results[2], results[3]):
        for k, ref in (("out", out), ("dlogp", dlogp), ("dbase", dbase), ("imp_sum", imp_sum), ("ema", ema)):
            same(r[k], ref, f"{k} of air_gauss_sample_bwd_nvil against air_nvil_parts")


@pytest.mark.parametrize("T,B", PC.HEADS_TB)
def test_Ga_heads_equal_the_stand_alone_launches_bit_for_bit(hip, T, B):
    """air_heads_fwd / _bwd with more than 8192 rows: the Gaussian workgroups of the forward sit at the cap (gauss_blocks = 2048) and the
    count body's virtual index starts behind them; every output equals the stand-alone launch's"""
    D, M = 4, T * B
    assert M > PC.CAP_ROWS
    gen = torch.Generator().manual_seed(1000 * T + B)
    pre = (torch.randn(M, 2 * D + 3, generator=gen) * 1.5).cuda()[:, :2 * D]
    eps, dsample, dkl = (torch.randn(M, D, generator=gen).cuda(), torch.randn(M, D, generator=gen).cuda(), torch.randn(M, generator=gen).cuda())
    logit, u = torch.randn(T, B, generator=gen).cuda(), torch.rand(T, B, generator=gen).cuda()
    prior = O.geometric_prior(AC.NSP, T).cuda()
    gauss, count = hip.heads_fwd(pre, eps, 0.5, 1, PC.PRIOR_A, logit, u, 0.75, 1e-3, prior)
    for got, ref, nm in zip(gauss, hip.gauss_sample_fwd(pre, eps, 0.5, 1, PC.PRIOR_A), ("loc", "scale", "sample", "kl_row")):
        AC.assert_bits(got, ref, f"heads_fwd T={T} B={B} {nm}")
    for got, ref, nm in zip(count, hip.presence_numsteps_fwd(logit, u, 0.75, 1e-3, prior), ("prob", "presence", "q", "kl", "logp", "step_weight")):
        AC.assert_bits(got, ref, f"heads_fwd T={T} B={B} {nm}")
    ka, kb = torch.rand(T, B, generator=gen).cuda() * 4, torch.rand(T, B, generator=gen).cuda() * 40
    dlogp = torch.randn(B, generator=gen).cuda()
    args = (count[0], count[1], prior, AC.KL_SCALE, ka, kb, AC.W_SCALE, dlogp, None, logit, 0.75, 1e-3)
    dpre, dlogit = hip.heads_bwd(pre, eps, 0.5, 1, PC.PRIOR_A, gauss[0], gauss[1], dsample, dkl, *args)
    AC.assert_bits(dpre, hip.gauss_sample_bwd(pre, eps, 0.5, 1, PC.PRIOR_A, gauss[0], gauss[1], dsample, dkl), f"heads_bwd T={T} B={B} dpre")
    AC.assert_bits(dlogit, hip.numsteps_presence_bwd(*args), f"heads_bwd T={T} B={B} dlogit")
    assert bool(torch.isfinite(dpre).all()) and bool(torch.isfinite(dlogit).all())


@pytest.mark.parametrize("entry,what,status", PC.GA_REFUSALS)
def test_Ga_refusals_write_nothing(hip, entry, what, status):
    name = "Ga_3x4_where"
    d, c = PC.ga_data(name), PC.GA[name]
    M, D = c["M"], c["D"]
    lib = hip.lib()
    st = Stage()
    if entry == "fwd":
        pre, eps = st.inp("pre", _pre_wide(d)), (None if what == "sample_no_eps" else st.inp("eps", d["eps"]))
        loc, scale, sample, kl = st.out("loc", (M, D)), st.out("scale", (M, D)), st.out("sample", (M, D)), st.out("kl_row", (M,))
        got = _fwd_launch(hip, st, d, c, pre, eps, loc, scale, sample, kl, ld_pre=2 * D - 1 if what == "ld_pre" else None,
                          loc_mode=2 if what == "loc_mode2" else None, M=0 if what == "M0" else None)
    elif entry in ("bwd", "bwd_nvil"):
        a = _bwd_args(st, d, c, "ds_ds2")
        if what == "ds_no_eps":
            a["eps"], a["dsample2"] = None, None
        if what == "ds2_no_eps":
            a["eps"], a["dsample"] = None, None
        head = _bwd_head(c, a, ld_pre=2 * D - 1 if what == "ld_pre" else None, ld_dpre=2 * D - 1 if what == "ld_dpre" else None,
                         M=0 if what == "M0" else None)
        if entry == "bwd":
            got = lib.air_gauss_sample_bwd(*head, c["guard"], None, 0, None, stream())
        else:
            nv = PC.nvil_inputs()
            B = nv["baseline"].shape[0]
            imp, base, logp = st.inp("imp_parts", nv["imp_parts"]), st.inp("baseline", nv["baseline"]), st.inp("logp", nv["logp"])
            out, dlogp, dbase = st.out("nvil_out", (4,)), st.out("dlogp", (B,)), st.out("dbaseline", (B,))
            got = lib.air_gauss_sample_bwd_nvil(*head, P(imp), 3, None, P(base), P(logp), P(out), P(dlogp), P(dbase), B, c["guard"], None,
                                                None, 0, None, stream())
    elif entry == "kl_fwd":
        loc, scale, kl = st.inp("loc", d["loc32"]), st.inp("scale", d["scale32"]), st.out("kl_row", (M,))
        got = lib.air_normal_kl_fwd(P(loc), P(scale), *c["prior4"], P(kl), 0, D, stream())
    else:
        loc, scale = st.inp("loc", d["loc32"]), st.inp("scale", d["scale32"])
        dloc, dscale = st.out("dloc", (M, D)), st.out("dscale", (M, D))
        got = lib.air_normal_kl_bwd(P(loc), P(scale), *c["prior4"], None, P(dloc), P(dscale), M, D, stream())
    assert got == status, (entry, what, got)
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Op
# ---------------------------------------------------------------------------------------------------------------
def _counters(c):
    gstep = torch.tensor([PC.GSTEP0], dtype=torch.int64).cuda() if c["counters"] in ("both", "no_rng") else None
    rng = torch.tensor([PC.i64(v) for v in PC.RNG0], dtype=torch.int64).cuda() if c["counters"] in ("both", "no_gstep") else None
    return gstep, rng


def _check_counters(gstep, rng):
    if gstep is not None:
        assert gstep.item() == PC.GSTEP0 + 1
    if rng is not None:
        assert rng.tolist() == [PC.i64(PC.RNG0[0]), PC.i64(PC.RNG0[1] + PC.RNG_INC)] and rng[1].item() == 2 ** 32 + 2      # the offset wraps


def _op_stage(d, off=()):
    st = Stage()
    bufs = {k: (st.inp(k, d[k], k in off) if k == "g" else st.state(k, d[k], k in off)) for k in PC.BUFS}
    return st, bufs


def _hyper(h):
    return h["decay"], h["momentum"], h["eps"], h["gscale"]


def _epilogue(hip, d, c, bufs, st, shadow, gstep=None, rng=None, shadow_off=False):
    h = d["h"]
    lr = torch.tensor([h["lr"]], dtype=torch.float32).cuda()
    p16 = st.out16("p_bf16", c["n"], shadow_off) if shadow else None
    head = (*(P(bufs[k]) for k in PC.BUFS), c["n_model"], c["n"], P(lr), h["tail"], *_hyper(h), P(gstep), P(rng), PC.RNG_INC)
    if shadow:
        return hip.lib().air_step_epilogue_shadow(*head, P(p16), stream()), p16
    return hip.lib().air_step_epilogue(*head, stream()), None


def _check_state(d, bufs, what):
    for k in ("p", "ms", "mg", "mom"):
        same(bufs[k], d["ref32"][k], f"{what} {k} against the float32 restatement")


@pytest.mark.parametrize("name", [n for n, c in PC.OP.items() if c["entry"] == "epilogue"])
def test_Op_step_epilogue_is_the_restatement_bit_for_bit(hip, name):
    d, c = PC.op_data(name), PC.OP[name]
    st, bufs = _op_stage(d, c["off"])
    gstep, rng = _counters(c)
    status, p16 = _epilogue(hip, d, c, bufs, st, c["shadow"], gstep, rng)
    assert status == 0
    st.untouched()
    _check_state(d, bufs, name)
    _check_counters(gstep, rng)
    if p16 is not None:
        src = bufs["p"].cpu().numpy().view(np.uint32)
        assert PC.bf16_mismatches(src, p16.cpu().numpy().view(np.uint16)) == 0, f"{name}: the shadow is not the cast of the updated p"
    if c["off"]:                                    # the scalar form an unaligned buffer forces against the aligned launch
        st2, bufs2 = _op_stage(d)
        assert _epilogue(hip, d, c, bufs2, st2, False)[0] == 0
        st2.untouched()
        for k in ("p", "ms", "mg", "mom"):
            same(bufs[k], bufs2[k], f"{name} {k} against the aligned launch")


@pytest.mark.parametrize("name", [n for n, c in PC.OP.items() if c["entry"] in ("rmsprop", "rmsprop_centered", "rmsprop_plain")])
def test_Op_rmsprop(hip, name):
    """the stand-alone update: one learning rate lr_dev[0] * lr_mult.  Centred: the restatement's bits; plain: float64 within
    fold_cases.RMS_TOL, the mg slot updated all the same"""
    d, c = PC.op_data(name), PC.OP[name]
    h = d["h"]
    st, bufs = _op_stage(d)
    lr = torch.tensor([h["lr"]], dtype=torch.float32).cuda()
    head = (*(P(bufs[k]) for k in PC.BUFS), c["n"], P(lr), h["tail"], h["decay"], h["momentum"], h["eps"])
    if c["entry"] == "rmsprop_centered":
        status = hip.lib().air_rmsprop_centered(*head, h["gscale"], stream())
    else:
        status = hip.lib().air_rmsprop(*head, int(c["entry"] == "rmsprop"), h["gscale"], stream())
    assert status == 0
    st.untouched()
    if c["entry"] != "rmsprop_plain":
        _check_state(d, bufs, name)
        return
    ref = PC.op_ref64(d, centred=False)
    for k in ("p", "ms", "mg", "mom"):
        assert_close(bufs[k], ref[k], *FC.RMS_TOL[k], f"{name} {k}", "Op")
    assert not np.array_equal(bufs["mg"].cpu().numpy(), d["mg"])


def _lstm_pointwise(gen, M=5, Hd=8):
    rn = lambda *s: torch.randn(*s, generator=gen).cuda()
    return torch.sigmoid(rn(M, 4 * Hd)), rn(M, Hd), rn(M, Hd), rn(M, Hd), rn(M, Hd), M, Hd


def _rider(hip, d, c, bufs, lo, hi):
    from attend_infer_repeat_amd import _lib
    h = d["h"]
    lr = torch.tensor([h["lr"]], dtype=torch.float32).cuda()
    act, c0, c1, dh, dc, M, Hd = _lstm_pointwise(torch.Generator().manual_seed(7))
    sl = _lib.AirRmspropSlice(*(bufs[k].data_ptr() for k in PC.BUFS), lo, hi, c["n_model"], lr.data_ptr(), h["tail"], h["decay"],
                              h["momentum"], h["eps"], h["gscale"])
    dg, dcp = torch.full((M, 4 * Hd), float("nan")).cuda(), torch.full((M, Hd), float("nan")).cuda()
    status = hip.lib().air_lstm_pointwise_bwd_opt(P(act), P(c0), P(c1), P(dh), None, P(dc), P(dg), P(dcp), M, Hd, ctypes.byref(sl), stream())
    dg0, dcp0 = torch.full((M, 4 * Hd), float("nan")).cuda(), torch.full((M, Hd), float("nan")).cuda()
    assert hip.lib().air_lstm_pointwise_bwd(P(act), P(c0), P(c1), P(dh), None, P(dc), P(dg0), P(dcp0), M, Hd, stream()) == 0
    torch.cuda.synchronize()
    AC.assert_bits(dg, dg0, "the carrier's own dgates"); AC.assert_bits(dcp, dcp0, "the carrier's own dc_prev")
    return status


@pytest.mark.parametrize("name", [n for n, c in PC.OP.items() if c["entry"] == "rider"])
def test_Op_rider_of_lstm_pointwise_bwd_opt(hip, name):
    d, c = PC.op_data(name), PC.OP[name]
    st, bufs = _op_stage(d)
    assert _rider(hip, d, c, bufs, *d["span"]) == 0
    st.untouched()
    _check_state(d, bufs, name)                     # (ref32 keeps the elements outside [lo, hi) as they were)


@pytest.mark.parametrize("name", ["Op_epi_planted_vec", "Op_epi_vec_tail10"])
def test_Op_every_carrier_agrees_with_every_other_bit_for_bit(hip, name):
    """one state through the vector epilogue, the scalar epilogue (p 4 bytes off), air_rmsprop segment by segment and the rider"""
    d, c = PC.op_data(name), PC.OP[name]
    h, n, nm = d["h"], c["n"], c["n_model"]
    got = {}
    st, bufs = _op_stage(d)
    assert _epilogue(hip, d, c, bufs, st, False)[0] == 0
    got["vector epilogue"] = bufs
    st, bufs = _op_stage(d, ("p",))
    assert _epilogue(hip, d, c, bufs, st, False)[0] == 0
    got["scalar epilogue"] = bufs
    st, bufs = _op_stage(d)
    lr = torch.tensor([h["lr"]], dtype=torch.float32).cuda()
    for lo, hi, mult in ((0, nm, 1.0), (nm, n, h["tail"])):
        assert hip.lib().air_rmsprop(*(P(bufs[k][lo:hi]) for k in PC.BUFS), hi - lo, P(lr), mult, h["decay"], h["momentum"], h["eps"], 1,
                                     h["gscale"], stream()) == 0
    got["air_rmsprop"] = bufs
    st, bufs = _op_stage(d)
    assert _rider(hip, d, c, bufs, 0, n) == 0
    got["rider"] = bufs
    torch.cuda.synchronize()
    for who, b in got.items():
        for k in ("p", "ms", "mg", "mom"):
            same(b[k], got["vector epilogue"][k], f"{name}: {k} of the {who} against the vector epilogue")
    _check_state(d, got["vector epilogue"], name)


def test_Op_shadow_two_bytes_off_is_refused(hip):
    name = "Op_epi_vec_script"
    d, c = PC.op_data(name), PC.OP[name]
    st, bufs = _op_stage(d)
    gstep, rng = _counters(c)
    status, p16 = _epilogue(hip, d, c, bufs, st, True, gstep, rng, shadow_off=True)
    assert p16.data_ptr() % 8 == 2 and status == PC.E_ALIGN
    st.untouched(written=False)
    assert gstep.item() == PC.GSTEP0 and rng.tolist() == [PC.i64(v) for v in PC.RNG0]


@pytest.mark.parametrize("name", list(PC.L2))
def test_Op_l2_grad_add(hip, name):
    d = PC.l2_data(name)
    c = d["case"]
    st = Stage()
    g, p = st.state("g", d["g"]), st.inp("p", d["p"])
    k = max(len(c["ranges"]), 1)
    lo = (ctypes.c_size_t * k)(*[r[0] for r in c["ranges"]])
    hi = (ctypes.c_size_t * k)(*[r[1] for r in c["ranges"]])
    assert hip.lib().air_l2_grad_add(P(g), P(p), lo, hi, len(c["ranges"]), PC.L2_WEIGHT, stream()) == c["status"]
    st.untouched(written=(c["status"] == 0))
    if c["status"] == 0:
        out = g.cpu().numpy()
        assert_close(out[d["inside"]], d["ref64"][d["inside"]], *PC.L2_TOL, name, "Op")
        same(out[~d["inside"]], d["g"][~d["inside"]], f"{name}: elements between the ranges")


# ---------------------------------------------------------------------------------------------------------------
# Bf
# ---------------------------------------------------------------------------------------------------------------
def _cast_ok(src_bits, out16, what):
    out = out16.cpu().numpy().view(np.uint16)
    bad = PC.bf16_mismatches(src_bits, out)
    if bad:
        rne = PC.bf16_rne(src_bits)
        i = int(np.flatnonzero(np.where(PC.is_nan32(src_bits), ~PC.is_nan16(out), out != rne))[0])
        raise AssertionError(f"{what}: {bad} of {len(src_bits)} casts differ; first: 0x{int(src_bits[i]):08x} -> 0x{int(out[i]):04x}, "
                             f"round-to-nearest-even gives 0x{int(rne[i]):04x}")


def _prologue_cvt(hip, st, x, x16, n):
    T, B, Hd = 3, 2, 4
    rng = torch.tensor([5, 0], dtype=torch.int64).cuda()
    gstep = torch.zeros(1, dtype=torch.int64).cuda()
    prior = torch.full((T + 1,), float("nan"), dtype=torch.float64).cuda()
    h0, c0 = st.inp("h0", np.arange(Hd, dtype=F32)), st.inp("c0", -np.arange(Hd, dtype=F32))
    ht, ct = st.out("h_tiled", (B, Hd)), st.out("c_tiled", (B, Hd))
    status = hip.lib().air_step_prologue_cvt(None, 0, None, 0, P(rng), P(gstep), 0, 0.3, 0.0, 1.0, 0.0, 1.0, P(prior), T, P(h0), P(c0), P(ht),
                                             P(ct), B, Hd, P(x), P(x16), n, stream())
    return status, prior, ht, ct, h0, c0


@pytest.mark.parametrize("name", list(PC.BF))
def test_Bf_casts_round_to_nearest_even_and_keep_nan(hip, name):
    c = PC.BF[name]
    src = PC.bf_source(name)
    n = len(src)
    st = Stage()
    if c["entry"] == "cast":
        x, x16 = st.inp_bits("x", src, c["src_off"]), st.out16("x_bf16", n, c["dst_off"])
        assert (x.data_ptr() % 16 == 0) == (not c["src_off"]) and (x16.data_ptr() % 8 == 0) == (not c["dst_off"])
        assert hip.lib().air_f32_to_bf16(P(x), P(x16), n, stream()) == 0
        st.untouched()
        _cast_ok(src, x16, name)
    elif c["entry"] == "cvt":
        x, x16 = st.inp_bits("x", src), st.out16("x_bf16", n)
        status, prior, ht, ct, h0, c0 = _prologue_cvt(hip, st, x, x16, n)
        assert status == 0
        st.untouched()
        _cast_ok(src, x16, name)
        assert bool(torch.isfinite(prior).all())
        AC.assert_bits(ht, h0[None].expand_as(ht).contiguous(), "h_tiled"); AC.assert_bits(ct, c0[None].expand_as(ct).contiguous(), "c_tiled")
    else:
        # the values pass through the epilogue unchanged: g = 0, mom = 0, momentum = 0 -> p - 0; the shadow is the cast of that p
        p = st.state("p", np.zeros(n, F32))
        p.view(torch.int32).copy_(torch.from_numpy(src.view(np.int32).copy()).cuda())
        g = st.inp("g", np.zeros(n, F32))
        ms, mg, mom = st.state("ms", np.ones(n, F32)), st.state("mg", np.zeros(n, F32)), st.state("mom", np.zeros(n, F32))
        p16 = st.out16("p_bf16", n)
        lr = torch.tensor([1e-3], dtype=torch.float32).cuda()
        assert hip.lib().air_step_epilogue_shadow(P(p), P(g), P(ms), P(mg), P(mom), n // 2, n, P(lr), 0.25, 0.9, 0.0, 1e-10, 1.0, None, None, 0,
                                                  P(p16), stream()) == 0
        torch.cuda.synchronize()
        assert PC.epilogue_form(n, n // 2) == ("vec" if "true" in c["kernel"] else "scalar")
        kept = p.cpu().numpy().view(np.uint32)
        nan = PC.is_nan32(src)
        assert (kept[~nan] == src[~nan]).all() and PC.is_nan32(kept[nan]).all(), f"{name}: p did not pass through unchanged"
        _cast_ok(src, p16, name)
        st.untouched()


@pytest.mark.parametrize("entry", ["cast", "cvt"])
def test_Bf_vector_casts_stride(hip, entry):
    n = PC.BF_STRIDED_N
    assert n // 4 > PC.CAP_ITEMS
    rng = np.random.default_rng(4)
    src = (rng.standard_normal(n).astype(F32) * np.exp(rng.uniform(-10, 10, n)).astype(F32)).view(np.uint32)
    st = Stage()
    x, x16 = st.inp_bits("x", src), st.out16("x_bf16", n)
    if entry == "cast":
        assert hip.lib().air_f32_to_bf16(P(x), P(x16), n, stream()) == 0
    else:
        assert _prologue_cvt(hip, st, x, x16, n)[0] == 0
    st.untouched()
    _cast_ok(src, x16, f"{entry} of {n} floats")


def test_Bf_refusals(hip):
    st = Stage()
    src = PC.bf_source("Bf_vec")[:8]
    x, x16 = st.inp_bits("x", src), st.out16("x_bf16", 8)
    assert hip.lib().air_f32_to_bf16(P(x), P(x16), 0, stream()) == PC.E_SHAPE
    assert hip.lib().air_f32_to_bf16(None, P(x16), 8, stream()) == PC.E_NULL
    x_off = st.inp_bits("x_off", src, True)
    assert _prologue_cvt(hip, st, x_off, x16, 8)[0] == PC.E_ALIGN
    assert _prologue_cvt(hip, Stage(), x, x16, 6)[0] == PC.E_SHAPE
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Ut
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PC.UT_SIZES)
def test_Ut_fill_and_axpby(hip, n):
    lib = hip.lib()
    st = Stage()
    out = st.out("fill", (n,))
    assert lib.air_fill(P(out), n, 2.5, stream()) == 0
    st.untouched()
    same(out, np.full(n, 2.5, F32), f"fill n={n}")
    for with_b in (False, True):
        a, b, alpha, beta = PC.axpby_inputs(n, with_b)
        st = Stage()
        da, db, res = st.inp("a", a), (st.inp("b", b) if with_b else None), st.out("out", (n,))
        assert lib.air_axpby(P(da), alpha, P(db), beta, P(res), n, stream()) == 0
        st.untouched()
        ref = FC.f32v(alpha) * a.astype(np.float64) + (FC.f32v(beta) * b.astype(np.float64) if with_b else 0.0)
        assert_close(res, ref, PC.AXPBY_RTOL, 0.0, f"axpby n={n} b={'given' if with_b else 'NULL'}", "Ut")


def test_Ut_zero_elements_write_nothing(hip):
    st = Stage()
    out, a = st.out("out", (4,)), st.inp("a", np.ones(4, F32))
    assert hip.lib().air_fill(P(out), 0, 2.5, stream()) == 0
    assert hip.lib().air_axpby(P(a), 1.0, None, 0.0, P(out), 0, stream()) == 0
    assert hip.lib().air_tile_rows(P(a), P(out), 0, 4, stream()) == PC.E_SHAPE
    assert hip.lib().air_colsum(P(a), 2, P(out), 1, 4, stream()) == PC.E_SHAPE            # ld < N
    st.untouched(written=False)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 255), (5, 257), (2051, 257)])
def test_Ut_tile_rows(hip, rows, cols):
    assert (rows, cols) != (2051, 257) or rows * cols > PC.CAP_ITEMS
    src = np.random.default_rng(cols).standard_normal(cols).astype(F32)
    st = Stage()
    s, out = st.inp("src", src), st.out("out", (rows, cols))
    assert hip.lib().air_tile_rows(P(s), P(out), rows, cols, stream()) == 0
    st.untouched()
    same(out, np.broadcast_to(src, (rows, cols)), f"tile_rows {rows} x {cols}")


@pytest.mark.parametrize("M,N", PC.COLSUM)
def test_Ut_colsum(hip, M, N):
    rng = np.random.default_rng(M * N)
    wide = np.full((M, N + 3), np.nan, F32)
    wide[:, :N] = rng.standard_normal((M, N)).astype(F32)
    st = Stage()
    x, out = st.inp("x", wide), st.out("out", (N,))
    assert hip.lib().air_colsum(P(x), N + 3, P(out), M, N, stream()) == 0
    st.untouched()
    same(out, PC.colsum32(wide[:, :N]), f"colsum {M} x {N}: the float32 sum in row order")
    x64 = wide[:, :N].astype(np.float64)
    err = np.abs(out.cpu().double().numpy() - x64.sum(0))
    bound = (M - 1) * PC.U32 * np.abs(x64).sum(0)
    assert (err <= bound).all()
    if M > 1:
        worst = float((err / bound).max())
        if "Ut" not in AC.WORST or worst > AC.WORST["Ut"][0]:
            AC.WORST["Ut"] = (worst, f"colsum {M} x {N}")
