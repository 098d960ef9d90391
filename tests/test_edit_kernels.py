"""GPU parity of the three stages that edit a parse, one launch at a time through the C ABI (run with -m gpu on an MI355X).  Cases,
float64 references, float32 restatements and bounds come from tests/edit_cases.py; tests/test_edit_cases_host.py holds them on the CPU.

Per launch: every operand is a window of a NaN-filled parent (integers: of an INT_FILL parent), every output a NaN-primed (integers:
INT_PRIMER) window of a SENTINEL-filled parent, every in-place buffer a window of a SENTINEL parent; after the launch the status is 0 and
every parent is unchanged to the bit outside what the launch owns.  A refused call returns its status and writes nothing.
  Rf  air_refine_step: J within CONST * 2^-24 * S of float64 (an image without a counted step: exactly -rec), J_trace exactly float32(J)
      in its own row only, the keep rule applied to the device's own J, best_* bit copies of all T rows, m / v / latent elementwise
      against the float64 rule, rows behind n untouched to the bit, the edges of the Adam step and of the guard, V = 1 / V = 2 by the
      alignment of `what`, the word copies the bits of the vector copies.
  Pn  air_prune_score per (band, image, mask) within its four-part bound, bands above 1024 and 2048 pixels, every T, a carve above
      64 KiB, NaN rows behind n the bits of zeros there, a NaN glimpse cell in exactly the masks and bands it reaches; air_prune_select:
      J_sub within its bound, every other output exact by the rule applied to the device's own J_sub, the planted ties and non-finite
      joints.
  Pr  air_propose_residual the bits of the rule on air_parse_render's canvas, within group X's bound of float64 away from the clamp
      points, res_parts within its bound; air_propose_pool / air_propose_source exact in every output.
The worst error / bound of each output is printed when the module finishes (pytest -s).

Worst error / bound on an MI355X (the float32 restatement on the CPU: 0.192 / 0.239 / 0.239 / 0.245 / 0.247 / 0.133 of the bound for
J / m / v / latent of the refine step, J_sub and the score): refine J 0.229, m 0.205, v 0.122, latent 0.244 (m and v below the
restatement: the refine file has no `fp contract(off)` and the device fuses b1 * m + (1 - b1) * g where the restatement rounds twice);
J_sub 0.247; score 0.140; residual against float64 0.202, res_parts 0.078.  Every bit bar holds.  No kernel changed."""
import numpy as np
import pytest
import torch

import attend_cases as AC
import edit_cases as EC
import readout_cases as RC
import warp_cases as WC
from attend_cases import SENTINEL
from attend_infer_repeat_amd import propose, prune
from test_readout_kernels import OwnerWin, P, Stage as _Stage, host, note, same, stream

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -5
OUTPUTS = ["rf_J", "rf_m", "rf_v", "rf_z", "sel_J", "score", "residual", "res_parts"]


@pytest.fixture(scope="module")
def L(gpu_device):
    from attend_infer_repeat_amd import hip as H
    return H.lib()


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    AC.print_worst("edit kernels", OUTPUTS)


class Stage(_Stage):
    def state(self, name, values, off=0):
        """an in-place buffer: its values as a window of a SENTINEL parent, `off` elements off a 16-byte boundary"""
        v = torch.as_tensor(np.ascontiguousarray(values))
        win = RC.Win(v.shape, off, SENTINEL, dtype=v.dtype)
        win.v.copy_(v)
        return self._add(name, win, "state")


def ptr(a, key, o):
    """the pointer of operand `key`: None if refused by name, `bytes` further if the case asks for it"""
    if key in o and o[key] is None:
        return None
    b = o.get("bytes")
    return P(a[key], b[1] if b and b[0] == key else 0)


def within(out, ref, S, kind, what, sel=None):
    out = host(out) if torch.is_tensor(out) else np.asarray(out)
    if sel is not None:
        out, ref, S = out[sel], np.asarray(ref)[sel], np.asarray(S)[sel]
    r = RC.worst_ratio(out, ref, S, EC.CONST[kind])
    print(f"\n  {what}: worst error / bound {r:.3g}")
    note(kind, r, what)
    assert r <= 1.0, f"{what}: worst error / bound {r:.3g}"


def f32(x):
    return float(F32(x))


# ---------------------------------------------------------------------------------------------------------------
# Rf: air_refine_step
# ---------------------------------------------------------------------------------------------------------------
RF_ITERS = 3
RF_STATE = EC.RF_UPDATED + ("best_J", "best_iter", "best_what", "best_where", "best_glimpse")


def _rf_launch(L, c, d, it=0, do_update=1, best=None, trace=True, pr=None, **o):
    """-> status, stage, device tensors, the host values the in-place buffers held before the launch"""
    T, B, A, G = (c[k] for k in ("T", "B", "A", "G"))
    off = {**c["off"], **o.get("off", {})}
    ad = {**EC.RF_ADAM, **o.get("adam", {})}
    pr = EC.priors32(o.get("prior", c["prior"])) if pr is None else pr
    rng = np.random.default_rng(7)
    before = {k: d[k] for k in EC.RF_UPDATED}
    before.update(best_J=np.full(B, 12345.0, F64), best_iter=np.full(B, 5, np.int32), best_what=rng.standard_normal((T, B, A)).astype(F32),
                  best_where=rng.standard_normal((T, B, 4)).astype(F32), best_glimpse=rng.standard_normal((T, B, G)).astype(F32))
    before.update(best or {})
    st = Stage()
    a = {k: st.inp(k, d[k]) for k in ("glimpse", "presence", "rec_parts", "dwhat", "dwhere", "where_loc")}
    a.update({k: st.state(k, before[k], off.get(k, 0)) for k in RF_STATE})
    a["J_trace"] = st.out("J_trace", (RF_ITERS, B)) if trace else None
    c1, c2 = o.get("c12", EC.bias_corrections(it, ad))
    dims = [o.get(k, c[k]) for k in ("T", "B", "A", "G")]
    p = lambda k: ptr(a, k, o)
    status = L.air_refine_step(p("what"), p("where"), p("glimpse"), p("presence"), p("rec_parts"), o.get("bands", c["bands"]), p("dwhat"),
                               p("dwhere"), p("where_loc"), *pr, p("m_what"), p("v_what"), p("m_where"), p("v_where"), f32(ad["lr_what"]),
                               f32(ad["lr_where"]), f32(ad["beta1"]), f32(ad["beta2"]), f32(ad["eps"]), c1, c2, f32(ad["guard"]),
                               o.get("iter", it), do_update, *dims, p("best_J"), p("best_iter"), p("best_what"), p("best_where"),
                               p("best_glimpse"), p("J_trace"), stream())
    return status, st, a, before


def _rf_check_kept(c, d, a, before, take, it, what):
    """the keep rule's outputs, given which images were taken: bit copies of all T rows (NaN payloads and -0.0 included)"""
    take = np.asarray(take, bool)
    assert (host(a["best_iter"]) == np.where(take, it, before["best_iter"])).all(), f"{what}: best_iter"
    for k, src in (("best_what", "what"), ("best_where", "where"), ("best_glimpse", "glimpse")):
        want = np.where(take.reshape(1, -1, 1), d[src], before[k])
        assert RC.same_bits(host(a[k]).view(np.int32), want.view(np.int32)) == 0, f"{what}: {k} is a bit copy where the iterate is taken"


def _rf_check_update(c, d, a, ref, what, lr_what=True, lr_where=True, images=None):
    counted = ref["mask"] if images is None else ref["mask"] & np.asarray(images, bool)[None, :]
    mask = np.broadcast_to(counted[..., None], d["what"].shape)
    mask4 = np.broadcast_to(counted[..., None], d["where"].shape)
    for base, m_, moved in (("what", mask, lr_what), ("where", mask4, lr_where)):
        r = ref[base]
        within(a["m_" + base], r["m"], r["S_m"], "rf_m", f"{what} m_{base}", m_)
        within(a["v_" + base], r["v"], r["S_v"], "rf_v", f"{what} v_{base}", m_)
        gone = ~np.broadcast_to(ref["mask"][..., None], d[base].shape)
        for k in (base, "m_" + base, "v_" + base):                   # the rows behind n keep their bits
            assert RC.same_bits(host(a[k])[gone].view(np.int32), d[k][gone].view(np.int32)) == 0, f"{what}: {k} behind n"
        if moved:
            within(a[base], r["z"], r["S_z"], "rf_z", f"{what} {base}", m_)
        else:
            assert RC.same_bits(host(a[base]).view(np.int32), d[base].view(np.int32)) == 0, f"{what}: {base} under lr = 0"


_RF_BASE = {}


def _rf_row(L, name):
    if name not in _RF_BASE:
        c, d = EC.RF_ROWS[name], EC.rf_data(name)
        status, st, a, before = _rf_launch(L, c, d)
        assert status == 0
        st.untouched()
        _RF_BASE[name] = (a, before)
    return _RF_BASE[name]


@pytest.mark.parametrize("name", list(EC.RF_ROWS))
def test_Rf_step(L, name):
    c, d = EC.RF_ROWS[name], EC.rf_data(name)
    pr = EC.priors32(c["prior"])
    a, before = _rf_row(L, name)
    ref = EC.rf_ref64(d, c, pr, 0)
    J = host(a["best_J"])
    within(J, ref["J"], ref["S_J"], "rf_J", f"{name} (V = {c['V']}) J")
    none = ref["n"] == 0
    assert (J[none] == -EC.f32_band_sum(d["rec_parts"]).astype(F64)[none]).all(), "no counted step: J is exactly -rec, the band-order float32 sum"
    trace = host(a["J_trace"])
    assert RC.same_bits(trace[0], J.astype(F32)) == 0 and np.isnan(trace[1:]).all(), "J_trace: float32(J) in row iter, no other row"
    _rf_check_kept(c, d, a, before, np.ones(c["B"], bool), 0, name)                     # iteration 0 takes whatever J is
    _rf_check_update(c, d, a, ref, name)
    if c["data"]:                                                                       # the same values on another load width / copy path
        peer, _ = _rf_row(L, c["data"])
        for k in RF_STATE:
            if k != "best_J" or "what" not in c["off"]:                                 # (another V adds in another order: J within its own bound)
                same(a[k], peer[k], f"{name}: {k} against the aligned launch")


def test_Rf_keep_rule(L):
    name = "Rf_3x5x12x16"
    c, d = EC.RF_ROWS[name], dict(EC.rf_data(name))
    rec = d["rec_parts"].copy()
    rec[1, 1], rec[0, 2], rec[2, 3] = np.nan, np.inf, -np.inf                            # J = NaN, -inf, +inf
    d["rec_parts"] = rec
    status, st, a, before = _rf_launch(L, c, d, do_update=0)
    assert status == 0
    st.untouched()
    J0 = host(a["best_J"]).copy()
    assert RC.classes(J0).tolist() == [0, 3, 2, 1, 0], "iteration 0 takes whatever J is, a NaN included"
    _rf_check_kept(c, d, a, before, np.ones(5, bool), 0, "iteration 0")
    for k in EC.RF_UPDATED:
        same(a[k], d[k], f"do_update = 0: {k}")
    pre = np.array([J0[0], 0.0, np.nan, 1e30, np.nextafter(J0[4], -np.inf)])
    results = []
    for trace in (True, False):
        status, st, a, before = _rf_launch(L, c, d, it=1, do_update=0, best=dict(best_J=pre), trace=trace, null_update=True,
                                           dwhat=None, dwhere=None, m_what=None, v_what=None, m_where=None, v_where=None)
        assert status == 0
        st.untouched()
        take = EC.keep_rule(J0, pre, 1)
        assert take.tolist() == [False, False, True, True, True], "J == best is not taken, a NaN J never, -inf over a NaN best, +inf over finite"
        same(host(a["best_J"]), np.where(take, J0, pre), "best_J: the device's own J where the iterate is taken")
        _rf_check_kept(c, d, a, before, take, 1, "iteration 1")
        for k in EC.RF_UPDATED:                                                         # all six update pointers NULL: untouched
            same(a[k], d[k], f"do_update = 0 without update pointers: {k}")
        if trace:
            tr = host(a["J_trace"])
            assert RC.same_bits(tr[1], J0.astype(F32)) == 0 and np.isnan(tr[[0, 2]]).all(), "only row iter of J_trace is written"
        results.append({k: host(a[k]).copy() for k in RF_STATE})
    for k in RF_STATE:
        same(results[0][k], results[1][k], f"J_trace = NULL: {k}")


def test_Rf_adam_edges(L):
    c, d = EC.RF_EDGE_ROW, EC.rf_edge_data()
    pr = EC.priors32("fixed")
    gd = F32(EC.RF_ADAM["guard"])
    status, st, a, _ = _rf_launch(L, c, d)
    assert status == 0
    st.untouched()
    ref = EC.rf_ref64(d, c, pr, 0)
    _rf_check_update(c, d, a, ref, "edges")
    what, where = host(a["what"]), host(a["where"])
    same(what[0, 0], d["what"][0, 0], "m = v = g = 0: the latent keeps its bits")
    assert (host(a["m_what"])[0, 0] == 0).all() and (host(a["v_where"])[0, 0] == 0).all()
    same(where[0, 0], np.array([gd, F32(2e-4), -gd, F32(-2e-4)], F32), "on +guard: left alone; -0.0: -guard; a shift inside: left alone")
    assert where[0, 1, 0] == gd and where[0, 1, 2] == -gd, "a scale landing inside (-guard, guard) becomes copysign(guard, .)"
    assert abs(where[0, 1, 1]) < gd, "a shift landing inside is left alone"
    # eps = 0 with v = 0: 0 / 0, the class of the plain formula position by position
    status, st, a, _ = _rf_launch(L, c, d, adam=dict(eps=0.0))
    assert status == 0
    st.untouched()
    ad0 = {**EC.RF_ADAM, "eps": 0.0}
    plain = EC.rf_restate32(d, c, pr, 0, c["V"], ad=ad0)                                # (image 0: g is 0 in float32 only, so the float32 formula)
    for base in ("what", "where"):
        got = host(a[base])
        assert (RC.classes(got) == RC.classes(plain[base])).all() and np.isnan(got[0, 0]).all(), f"eps = 0: {base}"
    _rf_check_update(c, d, a, EC.rf_ref64(d, c, pr, 0, ad=ad0), "edges, eps = 0", images=[False, True, True])
    # a prior scale of 0: the class of the plain formula
    pz = EC.priors32("fixed", what_p_scale=0.0)
    status, st, a, _ = _rf_launch(L, c, d, pr=pz)
    assert status == 0
    st.untouched()
    with np.errstate(all="ignore"):
        refz = EC.rf_ref64(d, c, pz, 0)
    assert (RC.classes(host(a["best_J"])) == RC.classes(refz["J"])).all(), "what_p_scale = 0: J"
    for k, key in (("what", "z"), ("m_what", "m"), ("v_what", "v")):
        assert (RC.classes(host(a[k])) == RC.classes(refz["what"][key])).all(), f"what_p_scale = 0: {k}"


@pytest.mark.parametrize("zero", ["lr_what", "lr_where"])
def test_Rf_zero_learning_rate(L, zero):
    name = "Rf_3x5x12x16"
    c, d = EC.RF_ROWS[name], EC.rf_data(name)
    status, st, a, _ = _rf_launch(L, c, d, adam={zero: 0.0})
    assert status == 0
    st.untouched()
    ref = EC.rf_ref64(d, c, EC.priors32(c["prior"]), 0, **{zero: 0.0})
    _rf_check_update(c, d, a, ref, f"{zero} = 0", lr_what=zero != "lr_what", lr_where=zero != "lr_where")


@pytest.mark.parametrize("tag,change,status", EC.RF_REFUSALS, ids=[r[0] for r in EC.RF_REFUSALS])
def test_Rf_refusals(L, tag, change, status):
    name = "Rf_3x5x6x9" if "prior" not in change else "Rf_3x5x12x16"                     # fixed prior: where_loc may be NULL
    c, d = EC.RF_ROWS[name], EC.rf_data(name)
    o = {k: v for k, v in change.items() if k != "prior"}
    got, st, a, _ = _rf_launch(L, c, d, **o)
    assert got == status, tag
    st.untouched(written=False)


def test_Rf_where_loc_may_be_null_under_a_fixed_shift_prior(L):
    c, d = EC.RF_ROWS["Rf_3x5x6x9"], EC.rf_data("Rf_3x5x6x9")
    status, st, a, _ = _rf_launch(L, c, d, where_loc=None)
    assert status == 0
    st.untouched()
    peer, _ = _rf_row(L, "Rf_3x5x6x9")
    for k in RF_STATE:
        same(a[k], peer[k], f"where_loc = NULL: {k}")


# ---------------------------------------------------------------------------------------------------------------
# Pn: air_prune_score
# ---------------------------------------------------------------------------------------------------------------
def _behind(d, c, fill):
    """the rows behind n of glimpse and where filled with `fill`"""
    T = c["T"]
    behind = np.arange(T)[:, None] >= d["n"][None, :]
    g, w = d["glimpse"].copy(), d["where"].copy()
    g[behind], w[behind] = fill, fill
    return {**d, "glimpse": g, "where": w}


def _score(L, name, allc, d=None, **o):
    c = EC.SC_ROWS[name]
    d = EC.sc_data(name) if d is None else d
    T, R = c["T"], c["R"]
    NB, RB = EC.unroll_bands(R, c["H"])
    off = c["off"]
    st = Stage()
    a = dict(glimpse=st.inp("glimpse", d["glimpse"], off.get("glimpse", 0)), where=st.inp("where", d["where"]),
             presence=st.inp("presence", d["presence"]), obs=st.inp("obs", d["obs"]), rec_sub=st.out("rec_sub", (NB, R, 1 << T)))
    dims = [o.get(k, c[k]) for k in ("T", "R", "H", "W", "h", "w")]
    p = lambda k: ptr(a, k, o)
    status = L.air_prune_score(p("glimpse"), p("where"), p("presence"), p("obs"), f32(EC.SC_MULT), f32(EC.SC_STD), allc, *dims,
                               NB + o.get("bands", 0), p("rec_sub"), stream())
    return status, st, a


@pytest.mark.parametrize("allc", [0, 1])
@pytest.mark.parametrize("name", list(EC.SC_ROWS))
def test_Pn_score(L, name, allc):
    c, d = EC.SC_ROWS[name], EC.sc_data(name)
    nref = d["nref"]
    status, st, a = _score(L, name, allc)
    assert status == 0
    st.untouched()
    got = host(a["rec_sub"]).copy()
    ref, S = EC.score_ref64(name, allc)
    within(got[:, :nref], ref, S, "score", f"{name} all_candidates = {allc}")            # (classes: the masks at or above 2^cb stay primed)
    rep = np.arange(c["R"]) % nref
    same(got, got[:, rep], f"{name}: the repeated images")
    status, st, a = _score(L, name, allc)
    assert status == 0
    same(a["rec_sub"], got, f"{name}: the same launch twice")
    if c.get("data"):
        status, st, b = _score(L, c["data"], allc)
        assert status == 0
        same(got, b["rec_sub"], f"{name}: scalar staging against vector staging")
    if not allc:                                                                        # rows behind n: NaN there, the bits of zeros there
        out = []
        for fill in (0.0, np.nan):
            status, st, a = _score(L, name, 0, _behind(d, c, fill))
            assert status == 0
            st.untouched()
            out.append(host(a["rec_sub"]).copy())
        same(out[1], out[0], f"{name}: NaN rows behind n against zeros there")
        same(out[0], got, f"{name}: zeros behind n against the finite rows")


@pytest.mark.parametrize("name,t", [("Sc_8x16", 1), ("Sc_33x32_one_band", 0), ("Sc_T4", 2)])
def test_Pn_score_nan_glimpse_cell(L, name, t):
    """all_candidates = 1, one NaN glimpse cell in step t of image 0: exactly the masks containing t are NaN in the bands its taps reach"""
    c, d = EC.SC_ROWS[name], EC.sc_data(name)
    T, H, W, h, w = (c[k] for k in ("T", "H", "W", "h", "w"))
    status, st, a = _score(L, name, 1)
    assert status == 0
    clean = host(a["rec_sub"]).copy()
    g = d["glimpse"].copy()
    g[t, 0, h // 2, w // 2] = np.nan
    status, st, a = _score(L, name, 1, {**d, "glimpse": g})
    assert status == 0
    st.untouched()
    got = host(a["rec_sub"])
    wh = d["where"][t, :1]
    ax, bx = WC.axis_ab(wh, "write", 0)
    ay, by = WC.axis_ab(wh, "write", 1)
    hole = np.zeros((1, h, w))
    hole[0, h // 2, w // 2] = 1.0
    reach = WC.warp64(hole, ax, bx, ay, by, W, H, np.zeros((1, H, W)))["out"][0] > 0
    hit = np.array([reach[r0:r1].any() for r0, r1 in EC.band_rows(c)])
    with_t = np.array([(m >> t) & 1 == 1 for m in range(1 << T)])
    want_nan = np.zeros(got.shape, bool)
    want_nan[:, 0, :] = hit[:, None] & with_t[None, :]
    assert hit.any() and (np.isnan(got) == want_nan).all(), f"{name}: NaN in the masks with step {t}, in the bands its taps reach"
    assert RC.same_bits(got[~want_nan], clean[~want_nan]) == 0, f"{name}: every other share keeps its bits"


@pytest.mark.parametrize("tag,change,status", EC.SC_REFUSALS, ids=[r[0] for r in EC.SC_REFUSALS])
def test_Pn_score_refusals(L, tag, change, status):
    got, st, a = _score(L, "Sc_8x16", 1, **change)
    assert got == status, tag
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Pn: air_prune_select
# ---------------------------------------------------------------------------------------------------------------
SEL_SHAPES = dict(J_sub=("R", "NM"), best_mask=("R",), num_objects_out=("R",), kept_step=("T", "R"), objective=("R",),
                  objective_start=("R",), evidence=("T", "R"), what_out=("T", "R", "A"), where_out=("T", "R", 4), glimpse_out=("T", "R", "G"),
                  score_out=("T", "R"))
SEL_DTYPE = dict(J_sub=torch.float64, objective=torch.float64, objective_start=torch.float64, evidence=torch.float64,
                 best_mask=torch.int32, num_objects_out=torch.int32, kept_step=torch.int32)


def _select(L, c, d, allc, pr=None, **o):
    dim = dict(T=c["T"], R=c["R"], A=c["A"], G=c["G"], NM=1 << c["T"])
    off = c["off"]
    pr = EC.priors32(c["prior"]) if pr is None else pr
    st = Stage()
    a = {k: st.inp(k, d[k], off.get(k, 0)) for k in EC.SEL_IN}
    for k in EC.SEL_OUT:
        a[k] = st.out(k, tuple(dim.get(s, s) for s in SEL_SHAPES[k]), off.get(k, 0), SEL_DTYPE.get(k, torch.float32))
    p = lambda k: ptr(a, k, o)
    status = L.air_prune_select(p("what"), p("where"), p("glimpse"), p("score"), p("presence"), p("where_loc"), *pr, p("prior"),
                                o.get("norm", c["norm"]), allc, p("rec_sub"), o.get("bands", c["bands"]), o.get("T", c["T"]), c["R"], c["A"],
                                c["G"], *[p(k) for k in EC.SEL_OUT], stream())
    return status, st, a


def _select_exact(c, d, a, allc, pr, what):
    """every output but J_sub, by the rule applied to the device's own J_sub"""
    J = host(a["J_sub"])
    want = prune.reference_select(d["what"], d["where"], d["glimpse"], d["score"], np.nan_to_num(d["presence"], nan=0.0), d["where_loc"], pr,
                                  d["prior"], c["norm"], allc, EC.f32_band_sum(d["rec_sub"]), J_sub=J)
    assert (host(a["best_mask"]) == want["best_mask"]).all(), f"{what}: best_mask"
    assert (host(a["num_objects_out"]) == want["num_objects"]).all() and (host(a["kept_step"]) == want["kept_step"]).all(), f"{what}: kept_step"
    same(host(a["objective"]), want["objective"], f"{what}: objective is J_sub[best]")
    same(host(a["objective_start"]), want["objective_start"], f"{what}: objective_start is J_sub[m0]")
    with np.errstate(invalid="ignore"):
        same(host(a["evidence"]), want["evidence"], f"{what}: evidence is the float64 difference, NaN from cb on")
    for k in ("what", "where", "glimpse", "score"):
        assert RC.same_bits(host(a[k + "_out"]).view(np.int32), np.ascontiguousarray(want[k]).view(np.int32)) == 0, f"{what}: {k}_out is a bit copy"
    return want


@pytest.mark.parametrize("allc", [0, 1])
@pytest.mark.parametrize("name", list(EC.SEL_ROWS))
def test_Pn_select(L, name, allc):
    c, d = EC.SEL_ROWS[name], EC.sel_data(name)
    pr = EC.priors32(c["prior"])
    status, st, a = _select(L, c, d, allc)
    assert status == 0
    st.untouched()
    J, S, n = EC.sel_ref64(d, c, pr, allc)
    within(a["J_sub"], J, S, "sel_J", f"{name} (V = {c['V']}) all_candidates = {allc} J_sub")
    _select_exact(c, d, a, allc, pr, name)
    if c["data"] and "what" not in c["off"]:                                            # a word copy: every bit of the aligned launch
        status, st, b = _select(L, EC.SEL_ROWS[c["data"]], d, allc)
        assert status == 0
        for k in EC.SEL_OUT:
            same(a[k], b[k], f"{name}: {k} against the aligned launch")
    if name == "Sel_3x5x12x16":                                                         # the table as given: normalize_prior = 0
        status, st, b = _select(L, c, d, allc, norm=0)
        assert status == 0
        Jn, Sn, _ = EC.sel_ref64(d, c, pr, allc, norm=0)
        within(b["J_sub"], Jn, Sn, "sel_J", f"{name} normalize_prior = 0 J_sub")


def test_Pn_select_planted(L):
    c, d = EC.SEL_PLANTED_ROW, EC.sel_planted_data()
    pr = EC.priors32(c["prior"])
    status, st, a = _select(L, c, d, 1)
    assert status == 0
    st.untouched()
    J, S, n = EC.sel_ref64(d, c, pr, 1)
    within(a["J_sub"], J, S, "sel_J", "planted J_sub")
    _select_exact(c, d, a, 1, pr, "planted")
    Jd, bm, idx = host(a["J_sub"]), host(a["best_mask"]), EC.SEL_PLANTED.index
    for tag in ("twins_tie", "start_ties", "twins_tie_n3"):
        assert Jd[idx(tag), 1:2].view(np.int64) == Jd[idx(tag), 2:3].view(np.int64), "two steps with the same latents: the same term bit for bit"
    for tag, m in EC.SEL_PLANTED_MASKS.items():
        assert bm[idx(tag)] == m, (tag, int(bm[idx(tag)]))
    assert np.isnan(host(a["objective"])[idx("all_nan")]) and bm[idx("start_nan")] != 7 and np.isposinf(host(a["objective"])[idx("one_pinf")])
    assert np.isneginf(Jd[idx("plain")][[3, 5, 6]]).all(), "prior[2] = 0: every mask of two steps is -inf"
    # a prior scale of 0: the class of the plain formula
    pz = EC.priors32("fixed", what_p_scale=0.0)
    status, st, a = _select(L, c, d, 1, pr=pz)
    assert status == 0
    with np.errstate(all="ignore"):
        Jz, _, _ = EC.sel_ref64(d, c, pz, 1)
    assert (RC.classes(host(a["J_sub"])) == RC.classes(Jz)).all(), "what_p_scale = 0"
    _select_exact(c, d, a, 1, pz, "what_p_scale = 0")


@pytest.mark.parametrize("tag,change,status", EC.SEL_REFUSALS, ids=[r[0] for r in EC.SEL_REFUSALS])
def test_Pn_select_refusals(L, tag, change, status):
    c, d = EC.SEL_ROWS["Sel_3x5x12x16"], EC.sel_data("Sel_3x5x12x16")                     # centred: where_loc is required
    got, st, a = _select(L, c, d, 1, **change)
    assert got == status, tag
    st.untouched(written=False)


def test_Pn_relabel_six_steps_over_the_passes(L):
    """air_prune_relabel at T = 6, R = 1025 inside windows: the rule of tests/test_relabel.py, bit for bit, and nothing else written"""
    T, R = 6, 1025
    rng = np.random.default_rng(1025)
    counts = rng.integers(-2, T + 3, R).astype(np.int32)
    n = np.clip(counts, 0, T)
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    src, ids = rng.standard_normal((T, R)).astype(F32), rng.integers(0, 256, (T, R)).astype(np.int32)
    src[0, 2], total = F32(-0.0), int(n.sum())
    want = dict(score=np.full((T, R), 7.5, F32), obj_score=np.full(total + 3, 7.5, F32), obj_step=np.full(total + 3, -5, np.int32))
    st = Stage()
    a = dict(src=st.inp("score_src", src), ids=st.inp("kept_step", ids), counts=st.inp("num_objects", counts), offsets=st.inp("offsets", offsets))
    out = {k: st.state(k, v) for k, v in want.items()}
    assert L.air_prune_relabel(P(a["src"]), P(a["ids"]), P(a["counts"]), P(a["offsets"]), T, R, P(out["score"]), P(out["obj_score"]),
                               P(out["obj_step"]), stream()) == 0
    st.untouched()
    for r in range(R):
        k, o = int(n[r]), int(offsets[r])
        want["score"][:k, r] = want["obj_score"][o:o + k] = src[:k, r]
        want["obj_step"][o:o + k] = ids[:k, r]
    for k in want:
        same(out[k], want[k], f"relabel: {k}")
    assert L.air_prune_relabel(P(a["src"]), P(a["ids"]), P(a["counts"]), P(a["offsets"]), 7, R, P(out["score"]), P(out["obj_score"]),
                               P(out["obj_step"]), stream()) == E_SHAPE


# ---------------------------------------------------------------------------------------------------------------
# Pr: air_propose_residual
# ---------------------------------------------------------------------------------------------------------------
def _residual(L, name, d=None, counts=None, presence=True, parts=True, hi=EC.RES_HI, **o):
    c = EC.SC_ROWS[name]
    d = EC.sc_data(name) if d is None else d
    T, R, H, W = c["T"], c["R"], c["H"], c["W"]
    NB, RB = EC.unroll_bands(R, H)
    st = Stage()
    a = dict(glimpse=st.inp("glimpse", d["glimpse"]), where=st.inp("where", d["where"]), presence=st.inp("presence", d["presence"] if presence else None),
             counts=st.inp("counts", counts), obs=st.inp("obs", d["obs"]), res=st.out("res", (R, H, W)),
             res_parts=st.out("res_parts", (NB, R)) if parts else None)
    dims = [o.get(k, c[k]) for k in ("T", "R", "H", "W", "h", "w")]
    p = lambda k: None if a[k] is None else ptr(a, k, o)
    status = L.air_propose_residual(p("glimpse"), p("where"), p("presence"), p("counts"), p("obs"), f32(EC.RES_MULT), float(hi), *dims,
                                    NB + o.get("bands", 0), p("res"), p("res_parts"), stream())
    return status, st, a


def _rendered(L, name, d, n):
    """mult * canvas of the rows t < n, by air_parse_render (its `reconstruction`) for the leading-ones chain of the same counts"""
    c = EC.SC_ROWS[name]
    T, R, H, W, h, w = (c[k] for k in ("T", "R", "H", "W", "h", "w"))
    chain = (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(F32)
    st = Stage()
    g, wh, pr, ob = st.inp("glimpse", d["glimpse"]), st.inp("where", d["where"]), st.inp("presence", chain), st.inp("obs", d["obs"])
    recon, area = st.out("reconstruction", (R, H, W)), st.out("area", (T, R), dtype=torch.int32)
    ow = OwnerWin((R, H, W))
    assert L.air_parse_render(P(g), P(wh), P(pr), P(ob), f32(EC.RES_MULT), f32(EC.SC_STD), 0.0, T, R, H, W, h, w, 1, P(recon), None, P(ow.v),
                              P(area), None, stream()) == 0
    st.untouched()
    return host(recon).copy()


@pytest.mark.parametrize("name", EC.RES_ROWS)
def test_Pr_residual(L, name):
    c, d = EC.SC_ROWS[name], EC.sc_data(name)
    T, R, nref = c["T"], c["R"], d["nref"]
    status, st, a = _residual(L, name, d)
    assert status == 0
    st.untouched()
    res, parts = host(a["res"]).copy(), host(a["res_parts"]).copy()
    recon = _rendered(L, name, d, d["n"])
    same(res, EC.residual_rule(d["obs"], recon, EC.RES_HI), f"{name}: res is the rule on air_parse_render's canvas, bit for bit")
    ref = EC.residual_ref64(name)
    away = ref["clear"] > 0                                                             # (the others: decided by the rule on the device's own canvas, above)
    err = np.abs(res[:nref].astype(F64) - ref["res"])
    r = float((err[away] / ref["bound"][away]).max())
    note("residual", r, name)
    assert r <= 1.0 and away.mean() > 0.9, f"{name}: res against float64, worst error / bound {r:.3g}"
    r = float((np.abs(parts[:, :nref] - ref["parts"]) / np.maximum(ref["parts_bound"], RC.TINY)).max())
    note("res_parts", r, name)
    assert r <= 1.0, f"{name}: res_parts, worst error / bound {r:.3g}"
    rep = np.arange(R) % nref
    same(res, res[rep], f"{name}: the repeated images")
    same(parts, parts[:, rep], f"{name}: res_parts of the repeated images")
    # rows behind n full of NaN: the bits of zeros there; res_parts = NULL: res keeps its bits
    for kw, what in ((dict(d=_behind(d, c, np.nan)), "NaN rows behind n"), (dict(d=_behind(d, c, 0.0)), "zeros behind n"),
                     (dict(d=d, parts=False), "res_parts = NULL")):
        status, st, b = _residual(L, name, **kw)
        assert status == 0
        st.untouched()
        same(b["res"], res, f"{name}: {what}")
    # counts given: clipped to 0 .. T, the bits of the presence form with the same counts; presence may then be NULL
    counts = d["n"].astype(np.int32)
    counts[d["n"] == 0], counts[d["n"] == T] = -3, T + 3
    for presence in (True, False):
        status, st, b = _residual(L, name, d, counts=counts, presence=presence)
        assert status == 0
        st.untouched()
        same(b["res"], res, f"{name}: num_objects_in, presence {'given' if presence else 'NULL'}")
        same(b["res_parts"], parts, f"{name}: res_parts under num_objects_in")


@pytest.mark.parametrize("hi", [np.inf, np.nan, 0.25])
def test_Pr_residual_clamp_and_nan_observation(L, hi):
    """clamp_hi = +inf clamps nothing; a NaN clamp_hi clamps nothing either (fminf drops a NaN operand); an observation NaN gives exactly 0"""
    name = "Sc_8x16"
    c, d = EC.SC_ROWS[name], EC.sc_data(name)
    obs = (F32(3.0) * d["obs"]).astype(F32)
    obs[0, 0, 0] = obs[2, 7, 15] = np.nan
    d = {**d, "obs": obs}
    status, st, a = _residual(L, name, d, hi=hi)
    assert status == 0
    st.untouched()
    res = host(a["res"])
    want = EC.residual_rule(obs, _rendered(L, name, d, d["n"]), hi)
    same(res, want, f"clamp_hi = {hi}")
    assert res[0, 0, 0] == 0 and res[2, 7, 15] == 0 and not np.isnan(res).any()
    assert res.max() > 1.0 if not hi == 0.25 else res.max() == 0.25


@pytest.mark.parametrize("tag,change,status", EC.RES_REFUSALS, ids=[r[0] for r in EC.RES_REFUSALS])
def test_Pr_residual_refusals(L, tag, change, status):
    if tag == "presence and counts":
        got, st, a = _residual(L, "Sc_8x16", presence=False)
    else:
        got, st, a = _residual(L, "Sc_8x16", **change)
    assert got == status, tag
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Pr: air_propose_pool, air_propose_source
# ---------------------------------------------------------------------------------------------------------------
POOL_IN = ("what", "where", "glimpse", "score", "presence", "counts", "source_in", "prop_what", "prop_where", "prop_glimpse", "prop_score", "prior")
POOL_OUT = ("pool_what", "pool_where", "pool_glimpse", "pool_score", "pool_presence", "pool_source", "pool_prior")


def _pool(L, T, P_, R, A, G, rnd=0, counts=False, presence=True, source=False, off=None, **o):
    d = EC.pool_data(T, P_, R, A, G)
    off = off or {}
    C = T + P_
    st = Stage()
    use = dict(d, counts=d["counts"] if counts else None, presence=d["presence"] if presence else None, source_in=d["source_in"] if source else None)
    a = {k: st.inp(k, use[k], off.get(k, 0)) for k in POOL_IN}
    shapes = dict(pool_what=(C, R, A), pool_where=(C, R, 4), pool_glimpse=(C, R, G), pool_score=(C, R), pool_presence=(C, R), pool_source=(C, R),
                  pool_prior=(C + 1,))
    for k in POOL_OUT:
        a[k] = st.out(k, shapes[k], off.get(k, 0), torch.int32 if k == "pool_source" else (torch.float64 if k == "pool_prior" else torch.float32))
    p = lambda k: None if a[k] is None else ptr(a, k, o)
    status = L.air_propose_pool(*[p(k) for k in POOL_IN], o.get("round", rnd), o.get("arg_T", T), o.get("arg_P", P_), R, A, G, *[p(k) for k in POOL_OUT],
                                stream())
    return status, st, a, d


def _pool_check(a, d, T, P_, rnd, counts, source, what):
    n = d["counts"] if counts else EC.leading_ones(d["presence"])
    want = propose.reference_pool(d["what"], d["where"], d["glimpse"], d["score"], n, d["prop_what"], d["prop_where"], d["prop_glimpse"],
                                  d["prop_score"], d["prior"], P_, round=rnd, source_in=d["source_in"] if source else None)
    for k in ("what", "where", "glimpse", "score", "presence"):
        assert RC.same_bits(host(a["pool_" + k]).view(np.int32), np.ascontiguousarray(want[k]).view(np.int32)) == 0, f"{what}: pool_{k}"
    assert (host(a["pool_source"]) == want["source"]).all(), f"{what}: pool_source"
    same(host(a["pool_prior"]), want["prior"], f"{what}: pool_prior, padded with exact zeros")


@pytest.mark.parametrize("A,G", EC.POOL_WIDTHS)
@pytest.mark.parametrize("T,P_,R", EC.POOL_SHAPES)
def test_Pr_pool_and_source(L, T, P_, R, A, G):
    for rnd, counts, presence, source in ((0, False, True, False), (3, True, True, True), (3, True, False, False), (0, False, True, True)):
        status, st, a, d = _pool(L, T, P_, R, A, G, rnd, counts, presence, source)
        assert status == 0
        st.untouched()
        _pool_check(a, d, T, P_, rnd, counts, source, f"pool {T}+{P_} x {R}, round {rnd}")
    # the provenance of the compacted rows; a kept_step of -1 and one of C are clipped: no read outside the pool (the window parents)
    C = T + P_
    rng = np.random.default_rng(R)
    kept = rng.integers(0, C, (C, R)).astype(np.int32)
    kept[0, 0], kept[C - 1, R - 1] = -1, C
    src = host(a["pool_source"]).copy()
    st = Stage()
    ps, ks, out = st.inp("pool_source", src), st.inp("kept_step", kept), st.out("source_out", (C, R), dtype=torch.int32)
    assert L.air_propose_source(P(ps), P(ks), C, R, P(out), stream()) == 0
    st.untouched()
    assert (host(out) == propose.reference_source(src, np.clip(kept, 0, C - 1))).all()
    for args in ((None, P(ks), C, R, P(out)), (P(ps), None, C, R, P(out)), (P(ps), P(ks), C, R, None)):
        assert L.air_propose_source(*args, stream()) == E_NULL
    assert L.air_propose_source(P(ps), P(ks), 0, R, P(out), stream()) == E_SHAPE and L.air_propose_source(P(ps), P(ks), 7, R, P(out), stream()) == E_SHAPE


@pytest.mark.parametrize("buf", ["what", "where", "glimpse", "score", "prop_what", "prop_where", "prop_glimpse", "prop_score", "pool_what",
                                 "pool_where", "pool_glimpse", "pool_score"])
def test_Pr_pool_row_buffers_misaligned(L, buf):
    T, P_, R, A, G = 3, 3, 5, 8, 16
    status, st, a, d = _pool(L, T, P_, R, A, G, 3, True, True, True, off={buf: 1})
    assert status == 0
    st.untouched()
    _pool_check(a, d, T, P_, 3, True, True, f"{buf} 4 bytes off")


@pytest.mark.parametrize("tag,change,status", EC.POOL_REFUSALS, ids=[r[0] for r in EC.POOL_REFUSALS])
def test_Pr_pool_refusals(L, tag, change, status):
    if tag == "presence and counts":
        got, st, a, d = _pool(L, 3, 3, 5, 8, 16, presence=False)
    else:
        got, st, a, d = _pool(L, 3, 3, 5, 8, 16, **{("arg_" + k if k in ("T", "P") else k): v for k, v in change.items()})
    assert got == status, tag
    st.untouched(written=False)
