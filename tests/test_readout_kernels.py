"""GPU parity of the evaluation read-outs, one launch at a time through the C ABI (run with -m gpu on an MI355X).  Cases, float64
references, float32 restatements and bounds come from tests/readout_cases.py; tests/test_readout_cases_host.py holds them on the CPU.

Per launch: every operand is a window of a NaN-filled parent (integers: of an INT_FILL parent), every output a NaN-primed (integers:
INT_PRIMER) window of a SENTINEL-filled parent; after the launch the status is 0, every output element is written and every parent is
unchanged to the bit outside what the launch owns.  A refused call returns its status and writes nothing.
  Iw  air_iw_logweight / air_iw_logposterior within CONST * 2^-24 * S of float64, non-finite results by class, num_steps exact, every
      launch misaligned onto V = 1 / V = 2 the bits of the launch with all three operands misaligned alike; air_iw_reduce within its
      bounds, the pinned non-finite blocks, the running totals the BITS of the float64 restatement of the stated order.
  Pp  air_particle_select exact in every output; air_particle_spread within one float32 rounding + the float64 term, presence_iw
      against the tail sums of air_iw_reduce's q_n, the pinned non-finite blocks.
  Gn  air_prior_latents: counts and presences exact, latents within the bound, the misaligned launches bit for bit; air_observe:
      mean the bits of mult * canvas, the noise the bits of air_rng_fill at the same counter, the scalar form the vector form's bits.
  Ps  air_parse_objects: counts, presences, offsets and the table exact, count_prob within one float32 rounding, score within T, boxes
      within their summands' bound; air_parse_render: every row first held to air_parse_render_form, reconstruction and layers
      within group X's bound of warp_cases.warp64, the canvas the bits of mult * air_canvas_unroll_fwd, owner exactly the rule applied
      to the launch's own layers, area exactly the count of owner.
The worst error / bound of each output is printed when the module finishes (pytest -s).

Worst error / bound on an MI355X (the float32 restatement on the CPU: 0.229 / 0.229 / 0.214 / 0.201 / 0.174 / 0.172 / 0.218 of the bound
for logw / logq / iw_bound / elbo / ess / q_n / latents): logw 0.207, logq 0.229, iw_bound 0.214, elbo 0.201, ess 0.127, q_n 0.167; spread
mean 0.986, std 0.970, presence_iw 0.985 (one float32 rounding of a float64 result), against the reduce's tail sums 0.085; latents 0.143,
observation 0.256; count_prob 0.957 (one rounding), score 0.322, boxes 0.494; reconstruction 0.372, layers 0.380, rec_parts 0.084.  Every
bit bar holds.  One kernel changed: particle_spread_kernel (a step one particle has: spread exactly 0; an infinite maximum shifts by 0)."""
import ctypes

import numpy as np
import pytest
import torch

import attend_cases as AC
import fold_cases as FC
import readout_cases as RC
import warp_cases as WC
from attend_cases import SENTINEL

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
OUTPUTS = ["logw", "logq", "iw_bound", "elbo", "ess", "q_n", "spread mean", "spread std", "presence_iw", "tail sums", "latents", "obs", "count_prob", "score", "boxes", "reconstruction", "layers", "rec_parts"]


@pytest.fixture(scope="module")
def L(gpu_device):
    from attend_infer_repeat_amd import hip as H
    return H.lib()


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    AC.print_worst("read-out kernels", OUTPUTS)


def P(t, byte_off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_off)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def host(t):
    return t.detach().cpu().numpy()


class Stage:
    """the operands of one launch on the device, and the check of everything the launch must not have touched"""

    def __init__(self):
        self.items = []

    def _add(self, name, win, kind):
        par, v = win.cuda()
        self.items.append((name, win, par, v, kind))
        return v

    def inp(self, name, values, off=0):
        return None if values is None else self._add(name, RC.in_win(values, off), "in")

    def out(self, name, shape, off=0, dtype=torch.float32):
        return self._add(name, RC.out_window(shape, off, dtype), "out")

    def state(self, name, values):
        """an in-place buffer: its values as a window of a SENTINEL parent"""
        v = torch.as_tensor(np.ascontiguousarray(values))
        win = RC.Win(v.shape, 0, SENTINEL, dtype=v.dtype)
        win.v.copy_(v)
        return self._add(name, win, "state")

    def untouched(self, written=True):
        torch.cuda.synchronize()
        for name, win, par, v, kind in self.items:
            if kind == "in" or not written:
                same = bits(par) == win.parent.view(torch.int32)
                assert bool(same.all()), f"{name}: {int((~same).sum())} words the launch must not write have changed"
                continue
            assert RC.surroundings_intact(win, par), f"{name}: written outside its window"
            if kind == "out":
                if v.dtype.is_floating_point:
                    pass                                            # (a NaN result is legitimate here: the tests compare classes)
                else:
                    assert bool((v != RC.INT_PRIMER).all()), f"{name}: an element was left unwritten"


def note(key, ratio, what):
    if key not in AC.WORST or ratio > AC.WORST[key][0]:
        AC.WORST[key] = (ratio, what)


def within(out, ref, S, kind, key, what):
    r = RC.worst_ratio(host(out) if torch.is_tensor(out) else out, ref, S, kind)
    print(f"\n  {what}: worst error / bound {r:.3g}")
    note(key, r, what)
    assert r <= 1.0, f"{what}: worst error / bound {r:.3g}"


def same(a, b, what):
    a = host(a) if torch.is_tensor(a) else np.asarray(a)
    b = host(b) if torch.is_tensor(b) else np.asarray(b)
    n = RC.same_bits(a, b)
    assert n == 0, f"{what}: {n} of {a.size} elements differ in their bits"


# ---------------------------------------------------------------------------------------------------------------
# Iw: the row kernels
# ---------------------------------------------------------------------------------------------------------------
SIX = ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale")
_ROW_RESULTS = {}


def _row_stage(name, off=None):
    c, d = RC.IW_ROWS[name], RC.iw_data(name)
    off = c["off"] if off is None else off
    st = Stage()
    a = {k: st.inp(k, d[k], off.get(k, 0)) for k in SIX}
    a.update(presence=st.inp("presence", d["presence"]), rec=st.inp("rec", d["rec"]), logp=st.inp("logp", d["logp"]),
             prior=st.inp("prior", d["table"]), logw=st.out("logw", (c["R"],)), n=st.out("num_steps", (c["R"],), dtype=torch.int32),
             logq=st.out("log_q", (c["R"],)))
    return st, a


def _logweight(L, c, a, **o):
    g = {**a, **{k: v for k, v in o.items() if k in a}}
    dims = [o.get(k, c[k]) for k in ("T", "R", "K", "A")]
    pr = [float(F32(v)) for v in RC.IW_PRIORS[c["prior"]]]
    return L.air_iw_logweight(*[g[k] if isinstance(g[k], ctypes.c_void_p) else P(g[k]) for k in SIX + ("presence", "rec", "logp", "prior")],
                              *dims, *pr, c["norm"], P(g["logw"]), P(g["n"]), stream())


def _logposterior(L, c, a, **o):
    g = {**a, **{k: v for k, v in o.items() if k in a}}
    dims = [o.get(k, c[k]) for k in ("T", "R", "K", "A")]
    return L.air_iw_logposterior(*[g[k] if isinstance(g[k], ctypes.c_void_p) else P(g[k]) for k in SIX + ("presence", "logp")], *dims,
                                 P(g["logq"]), stream())


def _run_rows(L, name):
    if name not in _ROW_RESULTS:
        c = RC.IW_ROWS[name]
        st, a = _row_stage(name)
        assert _logweight(L, c, a) == 0 and _logposterior(L, c, a) == 0
        st.untouched()
        _ROW_RESULTS[name] = (host(a["logw"]).copy(), host(a["logq"]).copy(), host(a["n"]).copy())
    return _ROW_RESULTS[name]


@pytest.mark.parametrize("name", list(RC.IW_ROWS))
def test_Iw_logweight_and_logposterior(L, name):
    c, ref = RC.IW_ROWS[name], RC.iw_ref64(name)
    logw, logq, n = _run_rows(L, name)
    assert (n == ref["n"]).all(), f"{name}: num_steps"
    within(logw, ref["logw"], ref["S_logw"], "logw", "logw", f"{name} (V = {c['V']}) log w")
    within(logq, ref["logq"], ref["S_logq"], "logq", "logq", f"{name} (V = {c['V']}) log q")
    if c["off"]:
        peer = _run_rows(L, RC.IW_BIT_PEERS[c["V"]])
        same(logw, peer[0], f"{name}: log w against the same values on V = {c['V']}")
        same(logq, peer[1], f"{name}: log q against the same values on V = {c['V']}")


ROW_REFUSALS = [(k, {k: None}, E_NULL) for k in SIX + ("presence", "rec", "logp", "prior", "logw", "n", "logq")] + [
    ("K=0", dict(K=0), E_SHAPE), ("T=0", dict(T=0), E_SHAPE), ("T=33", dict(T=33), E_SHAPE), ("R%K", dict(K=4), E_SHAPE),
    ("A=0", dict(A=0), E_SHAPE), ("where+4", dict(off={"where": 1}), E_ALIGN), ("where_loc+4", dict(off={"where_loc": 1}), E_ALIGN),
    ("where_scale+4", dict(off={"where_scale": 1}), E_ALIGN), ("what+2", dict(bytes="what"), E_ALIGN),
    ("what_scale+2", dict(bytes="what_scale"), E_ALIGN)]


@pytest.mark.parametrize("tag,change,status", ROW_REFUSALS, ids=[r[0] for r in ROW_REFUSALS])
def test_Iw_row_refusals(L, tag, change, status):
    name = "Iw_5x6x3x12"
    c = RC.IW_ROWS[name]
    st, a = _row_stage(name, change.get("off", {}))
    o = {k: v for k, v in change.items() if k not in ("off", "bytes")}
    if "bytes" in change:
        o[change["bytes"]] = P(a[change["bytes"]], 2)
    if tag not in ("rec", "prior", "logw", "n"):
        assert _logposterior(L, c, a, **o) == status, f"air_iw_logposterior {tag}"
    if tag != "logq":
        assert _logweight(L, c, a, **o) == status, f"air_iw_logweight {tag}"
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Iw: air_iw_reduce
# ---------------------------------------------------------------------------------------------------------------
def _reduce(L, lw, counts, steps, gt=None, acc=None, **o):
    (B, K), n, T = lw.shape, counts, steps
    st = Stage()
    a = dict(logw=st.inp("logw", lw.reshape(-1)), n=st.inp("num_steps", n.reshape(-1)), iw_bound=st.out("iw_bound", (B,)),
             elbo=st.out("elbo", (B,)), ess=st.out("ess", (B,)), q_n=st.out("q_n", (B, T + 1)), gt=st.inp("gt", gt),
             acc=None if acc is None else st.state("acc", np.asarray(acc, F64)))
    a.update({k: v for k, v in o.items() if k in a})
    status = L.air_iw_reduce(P(a["logw"]), P(a["n"]), o.get("T", T), o.get("R", B * K), o.get("K", K), P(a["iw_bound"]), P(a["elbo"]),
                             P(a["ess"]), P(a["q_n"]), P(a["gt"]), P(a["acc"]), stream())
    return status, st, a


@pytest.mark.parametrize("name", list(RC.RED_CASES))
def test_Iw_reduce(L, name):
    c, d = RC.RED_CASES[name], RC.red_data(name)
    ref = RC.red_ref64(d["logw"], d["n"], c["T"])
    status, st, a = _reduce(L, d["logw"], d["n"], c["T"])
    assert status == 0
    st.untouched()
    for k in ("iw_bound", "elbo", "ess", "q_n"):
        within(a[k], ref[k], ref["S_" + k], k, k, f"{name} {k}")
    q = host(a["q_n"]).astype(F64)
    for b in range(c["B"]):
        if RC.RED_KINDS[b % 5] == "equal" and c["K"] <= 200:
            assert host(a["ess"])[b] == c["K"], "equal weights: every w is exactly 1, the sums are integers"
        if RC.RED_KINDS[b % 5] == "outside" and c["K"] > 1:
            assert q[b].sum() < 0.9                                     # counts of -1 and T + 1 are counted nowhere


@pytest.mark.parametrize("name", list(RC.RED_NONFINITE))
def test_Iw_reduce_nonfinite_blocks(L, name):
    lw, iw, elbo, ess, q = RC.RED_NONFINITE[name]
    block = np.array([[-3000.0, -2999.0, -3001.0, -3000.5, -2998.0], lw, [-3000.0, -2999.0, -3001.0, -3000.5, -2998.0]], F32)
    n = np.array([RC.RED_NONFINITE_COUNTS] * 3, np.int32)
    status, st, a = _reduce(L, block, n, 2)
    assert status == 0
    st.untouched()
    got = [host(a["iw_bound"])[1], host(a["elbo"])[1], host(a["ess"])[1]] + list(host(a["q_n"])[1])
    for g, want in zip(got, [iw, elbo, ess] + q):
        assert np.isnan(g) if want == "nan" else g == want, (name, got)
    for k in ("iw_bound", "elbo", "ess", "q_n"):                       # the neighbours are untouched by it
        assert np.isfinite(host(a[k])[[0, 2]]).all()
        same(host(a[k])[0], host(a[k])[2], f"{name}: the images around the block")


@pytest.mark.parametrize("B", [1, 256, 257, 1000])
def test_Iw_accumulate_bits(L, B):
    """the totals are the BITS of the float64 restatement of the stated order on the launch's own per-image outputs"""
    T, K = 3, 2
    rng = np.random.default_rng(B)
    lw = (-3000.0 + rng.uniform(-2.0, 2.0, (B, K))).astype(F32)
    n = rng.integers(0, T + 1, (B, K)).astype(np.int32)
    lw[::7] = F32(-2999.5)
    n[::7] = [1, 3]                                                  # q_n[1] == q_n[3] == 0.5: the arg-max takes the smaller count
    gt = rng.integers(0, T + 1, B).astype(np.int32)
    gt[0::14], gt[7::14] = 1, 3
    acc0 = [1.5, -2.25, 1e6 + 0.125, 3.0, 17.0]
    status, st, a = _reduce(L, lw, n, T, gt=gt, acc=acc0)
    assert status == 0
    st.untouched()
    q = host(a["q_n"])
    assert (q[::7, 1] == q[::7, 3]).all() and (q[::7, 1] == 0.5).all()
    want = RC.accumulate64(host(a["iw_bound"]), host(a["elbo"]), host(a["ess"]), q, gt, acc0)
    same(a["acc"], want, f"B = {B}: the running totals")
    hits = int((RC.argmax_counts(q) == gt).sum())
    assert host(a["acc"])[3] == 3.0 + hits and hits != int((RC.argmax_counts(q, tie_to_larger=True) == gt).sum())
    # gt NULL with acc given: acc[3] stays; acc NULL: the per-image launch alone
    status, st2, a2 = _reduce(L, lw, n, T, acc=acc0)
    assert status == 0
    st2.untouched()
    want2 = RC.accumulate64(host(a2["iw_bound"]), host(a2["elbo"]), host(a2["ess"]), q, None, acc0)
    same(a2["acc"], want2, f"B = {B}: the running totals without gt")
    assert host(a2["acc"])[3] == 3.0
    status, st3, a3 = _reduce(L, lw, n, T)
    assert status == 0
    st3.untouched()
    for k in ("iw_bound", "elbo", "ess", "q_n"):
        same(a3[k], a[k], f"B = {B}: {k} with and without the totals")


RED_REFUSALS = [(k, {k: None}, E_NULL) for k in ("logw", "n", "iw_bound", "elbo", "ess", "q_n")] + [
    ("gt without acc", dict(), E_NULL), ("K=0", dict(K=0), E_SHAPE), ("T=0", dict(T=0), E_SHAPE), ("T=33", dict(T=33), E_SHAPE),
    ("R%K", dict(R=9), E_SHAPE)]


@pytest.mark.parametrize("tag,change,status", RED_REFUSALS, ids=[r[0] for r in RED_REFUSALS])
def test_Iw_reduce_refusals(L, tag, change, status):
    d = RC.red_data("Red_K2_B5_T3")
    gt = np.zeros(5, np.int32)
    got, st, a = _reduce(L, d["logw"], d["n"], 3, gt=gt, acc=None if tag == "gt without acc" else [0.0] * 5, **change)
    assert got == status
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Pp: air_particle_select
# ---------------------------------------------------------------------------------------------------------------
SEL = dict(T=32, B=4, K=80, A=8, G=12)


def _select_data():
    rng = np.random.default_rng(11)
    T, B, K, A, G = (SEL[k] for k in "TBKAG")
    R = B * K
    lw = rng.uniform(-20, -5, (B, K)).astype(F32)
    lq = rng.uniform(-3, 0, (B, K)).astype(F32)
    lw[0, 5] = lw[0, 69] = 1.0
    lq[0, 5] = lq[0, 69] = 0.5                                       # equal maxima on the same lane across the stride
    lw[1, 70] = lw[1, 5] = 2.0
    lq[1, 70] = lq[1, 5] = 0.25                                      # on different lanes
    lw[2, 3], lq[2, 3] = np.inf, -np.inf                             # criterion 1: NaN, skipped; criterion 0: +inf, a value
    lw[2, 9] = -np.inf
    lw[3] = np.nan
    return dict(log_w=lw, log_q=lq, n=rng.integers(0, T + 1, (B, K)).astype(np.int32), where=rng.standard_normal((T, R, 4)).astype(F32),
                what=rng.standard_normal((T, R, A)).astype(F32), pp=rng.uniform(size=(T, R)).astype(F32),
                glimpse=rng.standard_normal((T, R, G)).astype(F32))


def _select(L, d, criterion, off=None, moved=None, **o):
    """off: float offsets per buffer; moved: a buffer whose pointer is passed 2 bytes on; o: dimensions / buffers replaced"""
    T, B, K, A, G = (SEL[k] for k in "TBKAG")
    off = off or {}
    st = Stage()
    a = dict(log_w=st.inp("log_w", d["log_w"].reshape(-1)), log_q=st.inp("log_q", d["log_q"].reshape(-1)), n=st.inp("n", d["n"].reshape(-1)),
             where=st.inp("where", d["where"]), what=st.inp("what", d["what"], off.get("what", 0)), pp=st.inp("pp", d["pp"]),
             glimpse=st.inp("glimpse", d["glimpse"], off.get("glimpse", 0)), best=st.out("best_particle", (B,), dtype=torch.int32),
             score=st.out("best_score", (B,)), num=st.out("num_objects", (B,), dtype=torch.int32),
             deg=st.out("degenerate", (B,), dtype=torch.int32), where_sel=st.out("where_sel", (T, B, 4)),
             what_sel=st.out("what_sel", (T, B, A), off.get("what_sel", 0)), pp_sel=st.out("pp_sel", (T, B)),
             glimpse_sel=st.out("glimpse_sel", (T, B, G), off.get("glimpse_sel", 0)))
    g = {**a, **{k: v for k, v in o.items() if k in a}}
    order = ("log_w", "log_q", "n", "where", "what", "pp", "glimpse", "best", "score", "num", "deg", "where_sel", "what_sel", "pp_sel",
             "glimpse_sel")
    ptr = [P(g[k], 2 if k == moved else 0) for k in order]
    status = L.air_particle_select(*ptr[:7], o.get("T", T), o.get("R", B * K), o.get("K", K), o.get("A", A), o.get("G", G), criterion,
                                   *ptr[7:], stream())
    return status, st, a


@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("off", [None, "what", "glimpse", "what_sel", "glimpse_sel"])
def test_Pp_select_exact(L, criterion, off):
    T, B, K, A, G = (SEL[k] for k in "TBKAG")
    d = _select_data()
    status, st, a = _select(L, d, criterion, {off: 1} if off else None)
    assert status == 0
    st.untouched()
    best, score, num, deg = RC.select_ref(d["log_w"], d["log_q"], d["n"], criterion)
    assert best.tolist()[:2] == [5, 5] and deg.tolist() == [0, 0, 0, 1] and best[2] == (3 if criterion == 0 else best[2])
    same(a["best"], best, "best_particle"); same(a["num"], num, "num_objects"); same(a["deg"], deg, "degenerate")
    assert (host(a["score"]).view(np.uint32) == score.view(np.uint32)).all(), "best_score (an all-NaN image: the bits 0x7fc00000)"
    rows = np.arange(B) * K + best
    same(a["where_sel"], d["where"][:, rows], "where_sel"); same(a["what_sel"], d["what"][:, rows], "what_sel")
    same(a["pp_sel"], d["pp"][:, rows], "presence_prob_sel"); same(a["glimpse_sel"], d["glimpse"][:, rows], "glimpse_sel")


SEL_REFUSALS = [(k, {k: None}, 0, E_NULL) for k in ("log_w", "n", "where", "what", "pp", "glimpse", "best", "score", "num", "deg", "where_sel",
                                                     "what_sel", "pp_sel", "glimpse_sel")] + [
    ("criterion 1 without log_q", dict(log_q=None), 1, E_NULL), ("criterion 2", dict(), 2, E_SHAPE), ("K=0", dict(K=0), 0, E_SHAPE),
    ("T=33", dict(T=33), 0, E_SHAPE), ("R%K", dict(K=7), 0, E_SHAPE), ("G=0", dict(G=0), 0, E_SHAPE), ("what+2", dict(bytes="what"), 0, E_ALIGN)]


@pytest.mark.parametrize("tag,change,criterion,status", SEL_REFUSALS, ids=[r[0] for r in SEL_REFUSALS])
def test_Pp_select_refusals(L, tag, change, criterion, status):
    got, st, a = _select(L, _select_data(), criterion, moved=change.get("bytes"), **{k: v for k, v in change.items() if k != "bytes"})
    assert got == status
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Pp: air_particle_spread
# ---------------------------------------------------------------------------------------------------------------
def _spread(L, lw, counts, xs, steps, **o):
    (B, K), n, where, T = lw.shape, counts, xs, steps
    st = Stage()
    a = dict(logw=st.inp("log_w", lw.reshape(-1)), n=st.inp("num_steps", n.reshape(-1)), where=st.inp("where", where, o.get("where_off", 0)),
             mean=st.out("where_mean", (T, B, 4), o.get("mean_off", 0)), std=st.out("where_std", (T, B, 4)), pres=st.out("presence_iw", (T, B)))
    a.update({k: v for k, v in o.items() if k in a})
    status = L.air_particle_spread(P(a["logw"]), P(a["n"]), P(a["where"]), o.get("T", T), o.get("R", B * K), o.get("K", K), P(a["mean"]),
                                   P(a["std"]), P(a["pres"]), stream())
    return status, st, a


def _spread_within(out, ref, S, key, what):
    out, ref = host(out).astype(F64), np.asarray(ref, F64)
    assert (RC.classes(out) == RC.classes(ref)).all(), f"{what}: finite / NaN in other places than the reference"
    fin = np.isfinite(ref)
    err, bnd = np.abs(out[fin] - ref[fin]), RC.spread_bound(ref[fin], np.asarray(S)[fin])
    assert (err[bnd == 0] == 0).all(), f"{what}: differs where the bound is zero"
    r = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
    print(f"\n  {what}: worst error / bound {r:.3g}")
    note(key, r, what)
    assert r <= 1.0, f"{what}: worst error / bound {r:.3g}"


@pytest.mark.parametrize("name", list(RC.SPREAD_CASES))
def test_Pp_spread(L, name):
    c, d = RC.SPREAD_CASES[name], RC.spread_data(name)
    T, B, K = c["T"], c["B"], c["K"]
    ref = RC.spread_ref64(d["logw"], d["n"], d["where"], T)
    status, st, a = _spread(L, d["logw"], d["n"], d["where"], T)
    assert status == 0
    st.untouched()
    _spread_within(a["mean"], ref["mean"], ref["S_mean"], "spread mean", f"{name} where_mean")
    _spread_within(a["std"], ref["std"], ref["S_std"], "spread std", f"{name} where_std")
    _spread_within(a["pres"], ref["presence_iw"], ref["S_presence_iw"], "presence_iw", f"{name} presence_iw")
    for b, p in d["planted"].items():
        assert np.isnan(host(a["mean"])[p["empty"], b]).all() and np.isnan(host(a["std"])[p["empty"], b]).all()
        assert host(a["pres"])[p["empty"], b] == 0.0, "a step no particle has: presence_iw exactly 0"
        assert (host(a["std"])[p["single"], b] == 0.0).all(), "a step one particle has: the spread is exactly 0"
        same(host(a["mean"])[p["single"], b], d["where"].reshape(T, B, K, 4)[p["single"], b, p["lone"]], "a step one particle has: its bits")
    # against the tail sums of air_iw_reduce's q_n on the same log-weights and counts, within the sum of the two outputs' bounds
    status, st2, r = _reduce(L, d["logw"], d["n"], T)
    assert status == 0
    red = RC.red_ref64(d["logw"], d["n"], T)
    q, bq = host(r["q_n"]).astype(F64), RC.bound("q_n", red["S_q_n"])
    worst = 0.0
    for t in range(T):
        tail, bnd = q[:, t + 1:].sum(1), bq[:, t + 1:].sum(1) + RC.spread_bound(ref["presence_iw"][t], ref["S_presence_iw"][t])
        err = np.abs(host(a["pres"])[t].astype(F64) - tail)
        assert (err[bnd == 0] == 0).all()
        worst = max(worst, float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0)
    print(f"\n  {name} presence_iw against the tail sums of q_n: worst error / bound {worst:.3g}")
    note("tail sums", worst, name)
    assert worst <= 1.0


def test_Pp_spread_nonfinite_blocks(L):
    """the reduce's convention: mean and spread NaN throughout, presence_iw the class of the tail sums of q_n"""
    T = 2
    n = np.array([RC.RED_NONFINITE_COUNTS] * 3, np.int32)
    where = np.random.default_rng(5).standard_normal((T, 15, 4)).astype(F32)
    want = {"all_ninf": ["nan", "nan"], "one_pinf": ["nan", 0.0], "one_nan": ["nan", "nan"]}
    for name, (lw, *_rest) in RC.RED_NONFINITE.items():
        block = np.array([[-3000.0, -2999.0, -3001.0, -3000.5, -2998.0], lw, [-3000.0, -2999.0, -3001.0, -3000.5, -2998.0]], F32)
        status, st, a = _spread(L, block, n, where, T)
        assert status == 0
        st.untouched()
        assert np.isnan(host(a["mean"])[:, 1]).all() and np.isnan(host(a["std"])[:, 1]).all(), name
        for t in range(T):
            g = host(a["pres"])[t, 1]
            assert np.isnan(g) if want[name][t] == "nan" else g == want[name][t], (name, t, g)
        _, _, r = _reduce(L, block, n, T)
        q = host(r["q_n"]).astype(F64)
        for t in range(T):
            assert RC.classes(q[1, t + 1:].sum()) == RC.classes(host(a["pres"])[t, 1]), (name, t)
        for k in ("mean", "std", "pres"):
            assert np.isfinite(host(a[k])[:, [0, 2]]).all(), name


SPR_REFUSALS = [(k, {k: None}, E_NULL) for k in ("logw", "n", "where", "mean", "std", "pres")] + [
    ("K=0", dict(K=0), E_SHAPE), ("T=0", dict(T=0), E_SHAPE), ("T=33", dict(T=33), E_SHAPE), ("R%K", dict(K=4), E_SHAPE),
    ("where+4", dict(where_off=1), E_ALIGN), ("where_mean+4", dict(mean_off=1), E_ALIGN)]


@pytest.mark.parametrize("tag,change,status", SPR_REFUSALS, ids=[r[0] for r in SPR_REFUSALS])
def test_Pp_spread_refusals(L, tag, change, status):
    d = RC.spread_data("Spr_K5_B5_T3")
    got, st, a = _spread(L, d["logw"], d["n"], d["where"], 3, **change)
    assert got == status
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Gn: air_prior_latents
# ---------------------------------------------------------------------------------------------------------------
_GEN_RESULTS = {}


def _latents(L, steps, rows, width, tab, uu, nin, ew, ewh, guard, off=None, **o):
    T, R, A, table, u, n_in, eps_what, eps_where = steps, rows, width, tab, uu, nin, ew, ewh
    off = off or {}
    st = Stage()
    a = dict(table=st.inp("table", table), u=st.inp("u", u), n_in=st.inp("n_in", n_in), eps_what=st.inp("eps_what", eps_what, off.get("eps_what", 0)),
             eps_where=st.inp("eps_where", eps_where, off.get("eps_where", 0)), what=st.out("what", (T, R, A), off.get("what", 0)),
             where=st.out("where", (T, R, 4), off.get("where", 0)), presence=st.out("presence", (T, R)),
             n=st.out("num_objects", (R,), dtype=torch.int32))
    g = {**a, **{k: v for k, v in o.items() if k in a}}
    pr = [float(F32(v)) for v in RC.GEN_PRIORS]
    ptr = {k: (g[k] if isinstance(g[k], ctypes.c_void_p) else P(g[k])) for k in g}
    status = L.air_prior_latents(ptr["table"], ptr["u"], ptr["n_in"], ptr["eps_what"], ptr["eps_where"], *pr, float(F32(guard)), o.get("T", T),
                                 o.get("R", R), o.get("A", A), ptr["what"], ptr["where"], ptr["presence"], ptr["n"], stream())
    return status, st, a


def _run_gen(L, name):
    if name not in _GEN_RESULTS:
        c, d = RC.GEN_ROWS[name], RC.gen_data(name)
        status, st, a = _latents(L, c["T"], c["R"], c["A"], d["table"], d["u"], None, d["eps_what"], d["eps_where"], RC.GEN_GUARD, c["off"])
        assert status == 0
        st.untouched()
        _GEN_RESULTS[name] = {k: host(a[k]).copy() for k in ("what", "where", "presence", "n")}
    return _GEN_RESULTS[name]


@pytest.mark.parametrize("name", list(RC.GEN_ROWS))
def test_Gn_prior_latents(L, name):
    c, d = RC.GEN_ROWS[name], RC.gen_data(name)
    out = _run_gen(L, name)
    n = RC.count_by_inversion(d["table"], d["u"], c["T"])
    ref = RC.latents_ref64(d, c["T"], RC.GEN_GUARD, n)
    same(out["n"], n, f"{name} num_objects")
    same(out["presence"], ref["presence"], f"{name} presence")
    within(out["what"], ref["what"], ref["S_what"], "latents", "latents", f"{name} (V = {c['V']}) what")      # absent steps like the others
    free = ~ref["guarded"]
    within(out["where"][free], ref["where"][free], ref["S_where"][free], "latents", "latents", f"{name} where")
    assert (out["where"][ref["guarded"]].astype(F64) == ref["where"][ref["guarded"]]).all(), f"{name}: a guarded scale is +-guard exactly"
    if c["R"] >= 5:
        assert ref["guarded"].sum() >= 2 and 0 < out["where"][0, 3, 1] < RC.GEN_GUARD      # a shift component inside the guard is left alone
    if c["off"]:
        peer = _run_gen(L, RC.GEN_BIT_PEERS[c["V"]])
        same(out["what"], peer["what"], f"{name}: what against the same values on V = {c['V']}")
        same(out["where"], peer["where"], f"{name}: where")


def test_Gn_prior_latents_boundaries_and_clipped_counts(L):
    T, A = 3, 4
    rng = np.random.default_rng(2)
    R = len(RC.DYADIC_U)
    ew, ewh = rng.standard_normal((T, R, A)).astype(F32), rng.standard_normal((T, R, 4)).astype(F32)
    status, st, a = _latents(L, T, R, A, np.array(RC.DYADIC_TABLE), np.array(RC.DYADIC_U, F32), None, ew, ewh, 0.0)
    assert status == 0
    st.untouched()
    assert host(a["n"]).tolist() == RC.DYADIC_N, "u on a cumulative boundary counts the step (cum <= thresh); u = 0; the float32 below 1"
    n_in = np.array([-3, T + 3, 0, T, 1, 2], np.int32)
    status, st, b = _latents(L, T, R, A, np.array(RC.DYADIC_TABLE), np.array(RC.DYADIC_U, F32), n_in, ew, ewh, 0.0)
    assert status == 0
    st.untouched()
    assert host(b["n"]).tolist() == [0, T, 0, T, 1, 2], "num_objects_in is clipped to 0 .. T and takes precedence over the table"
    same(b["presence"], (np.arange(T)[:, None] < np.array([0, T, 0, T, 1, 2])[None, :]).astype(F32), "presence")
    same(b["what"], a["what"], "what does not depend on the count")
    same(b["where"], a["where"], "where does not depend on the count")
    status, st, e = _latents(L, T, R, A, None, None, n_in, ew, ewh, 0.0)
    assert status == 0
    same(e["n"], b["n"], "counts given without a table")


GEN_REFUSALS = [(k, {k: None}, E_NULL) for k in ("eps_what", "eps_where", "what", "where", "presence", "n", "table", "u")] + [
    ("T=0", dict(T=0), E_SHAPE), ("T=33", dict(T=33), E_SHAPE), ("R=0", dict(R=0), E_SHAPE), ("A=0", dict(A=0), E_SHAPE),
    ("eps_where+4", dict(off={"eps_where": 1}), E_ALIGN), ("where+4", dict(off={"where": 1}), E_ALIGN), ("eps_what+2", dict(bytes="eps_what"), E_ALIGN)]


@pytest.mark.parametrize("tag,change,status", GEN_REFUSALS, ids=[r[0] for r in GEN_REFUSALS])
def test_Gn_prior_latents_refusals(L, tag, change, status):
    c, d = RC.GEN_ROWS["Gn_3x7x50"], RC.gen_data("Gn_3x7x50")
    o = {k: v for k, v in change.items() if k not in ("off", "bytes")}
    if "bytes" in change:
        st = Stage()
        moved = st.inp("moved", d[change["bytes"]])
        o[change["bytes"]] = P(moved, 2)
    got, st, a = _latents(L, c["T"], c["R"], c["A"], d["table"], d["u"], None, d["eps_what"], d["eps_where"], 0.0, change.get("off"), **o)
    assert got == status
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Gn: air_observe
# ---------------------------------------------------------------------------------------------------------------
def _observe(L, canvas, mult, std, base, lo, hi, off=(0, 0, 0), state=True, n=None, canvas_ptr=None):
    """off: float offsets of canvas / mean_out / obs_out, None: that output is NULL"""
    st = Stage()
    c = st.inp("canvas", canvas, off[0])
    s = st.inp("state", np.array([RC.OBS_SEED, RC.OBS_OFFSET], np.int64)) if state else None
    mean = None if off[1] is None else st.out("mean_out", (len(canvas),), off[1])
    obs = None if off[2] is None else st.out("obs_out", (len(canvas),), off[2])
    status = L.air_observe(canvas_ptr(c) if canvas_ptr else P(c), float(F32(mult)), float(F32(std)), P(s), ctypes.c_uint64(base), float(lo),
                           float(hi), P(mean), P(obs), ctypes.c_size_t(len(canvas) if n is None else n), stream())
    return status, st, mean, obs


def _canvas(n, seed=0):
    return np.random.default_rng(100 + n + seed).uniform(0.0, 1.0, n).astype(F32)


@pytest.mark.parametrize("n", RC.OBS_N)
@pytest.mark.parametrize("base", [0, 7, 2 ** 32 + 5])
def test_Gn_observe_against_float64_and_the_scalar_form(L, n, base):
    canvas, mult, std, lo, hi = _canvas(n), 1.7, 0.3, 0.05, 1.5
    mean_ref, obs_ref, bnd = RC.observe_ref(canvas, mult, std, base, lo, hi)
    status, st, mean, obs = _observe(L, canvas, mult, std, base, lo, hi)
    assert status == 0
    st.untouched()
    same(mean, mean_ref, f"n = {n}: mean, the bits of mult * canvas")
    err = np.abs(host(obs).astype(F64) - obs_ref)
    r = float((err / bnd).max())
    note("obs", r, f"n = {n}, counter_base = {base}")
    assert r <= 1.0, f"n = {n}: the observation, worst error / bound {r:.3g}"
    assert ((host(obs) == F32(lo)).any() or (host(obs) == F32(hi)).any()) or n < 100
    for k in range(3):                                                # each buffer in turn 4 bytes off: the scalar form, the same quads
        off = tuple(1 if i == k else 0 for i in range(3))
        status, st2, mean2, obs2 = _observe(L, canvas, mult, std, base, lo, hi, off)
        assert status == 0
        st2.untouched()
        same(mean2, mean, f"n = {n}: the scalar form's mean ({off})")
        same(obs2, obs, f"n = {n}: the scalar form's observation ({off})")


@pytest.mark.parametrize("base", [7, 2 ** 32 + 5])
def test_Gn_observe_draws_the_numbers_of_the_noise_fill(L, base):
    n = 4 * 625 + 3
    status, st, mean, obs = _observe(L, np.zeros(n, F32), 1.0, 1.0, base, RC.NAN, RC.NAN)
    assert status == 0
    st.untouched()
    same(obs, host(FC.philox_normals(RC.OBS_SEED, RC.OBS_OFFSET + base, n)), f"counter_base = {base}: 0 + 1 * z is z")


def test_Gn_observe_without_noise_null_outputs_and_nan_bounds(L):
    n = 4 * 625 + 3
    canvas = _canvas(n, 1)
    canvas[[2, 5, 2501]] = RC.NAN                                      # one in a full quad, one in the second, one in the cut quad
    mult, lo, hi = 1.7, 0.2, 1.2
    m32 = (F32(mult) * canvas).astype(F32)
    for off in [(0, 0, 0), (1, 0, 0)]:
        # std = 0: obs is the clamped mean, state NULL is accepted; a NaN pixel under a finite clamp comes out as lo (fmaxf drops the NaN)
        status, st, mean, obs = _observe(L, canvas, mult, 0.0, 0, lo, hi, off, state=False)
        assert status == 0
        st.untouched()
        same(mean, m32, "mean")
        same(obs, RC.observe_ref(canvas, mult, 0.0, 0, lo, hi, noise=False)[1].astype(F32), "std = 0: the clamped mean")
        assert (host(obs)[[2, 5, 2501]] == F32(lo)).all()
        status, st, mean, obs = _observe(L, canvas, mult, 0.0, 0, RC.NAN, RC.NAN, off, state=False)
        assert status == 0
        same(obs, mean, "std = 0, no clamp: obs is mean bit for bit")
        for lo_, hi_ in [(RC.NAN, hi), (lo, RC.NAN)]:
            status, st, mean, obs = _observe(L, canvas, mult, 0.0, 0, lo_, hi_, off, state=False)
            assert status == 0
            same(obs, RC.observe_ref(canvas, mult, 0.0, 0, lo_, hi_, noise=False)[1].astype(F32), f"clamp ({lo_}, {hi_})")
        # with noise a NaN pixel is still lo; a NaN lo: hi
        status, st, mean, obs = _observe(L, canvas, mult, 0.3, 0, lo, hi, off)
        assert status == 0 and (host(obs)[[2, 5, 2501]] == F32(lo)).all()
        status, st, mean, obs = _observe(L, canvas, mult, 0.3, 0, RC.NAN, hi, off)
        assert status == 0 and (host(obs)[[2, 5, 2501]] == F32(hi)).all()
        # mean_out NULL; obs_out NULL is the no-noise path even with std != 0 (no state needed)
        status, st, _, obs3 = _observe(L, canvas, mult, 0.3, 0, lo, hi, (off[0], None, 0))
        assert status == 0
        st.untouched()
        status, st, _, obs4 = _observe(L, canvas, mult, 0.3, 0, lo, hi, (0, 0, 0))
        same(obs3, obs4, "mean_out NULL changes nothing in obs")
        status, st, mean5, _ = _observe(L, canvas, mult, 0.3, 0, lo, hi, (off[0], 0, None), state=False)
        assert status == 0
        st.untouched()
        same(mean5, m32, "obs_out NULL: the mean alone")


def test_Gn_observe_refusals(L):
    canvas = _canvas(9)
    for kw, status in [(dict(off=(0, None, None)), E_NULL), (dict(state=False), E_NULL), (dict(n=0), E_SHAPE),
                       (dict(canvas_ptr=lambda c: P(c, 2)), E_ALIGN), (dict(canvas_ptr=lambda c: None), E_NULL)]:
        got, st, mean, obs = _observe(L, canvas, 1.7, 0.3, 0, 0.0, 1.0, **kw)
        assert got == status, kw
        st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Ps: air_parse_objects
# ---------------------------------------------------------------------------------------------------------------
TABLE = ("obj_image", "obj_step", "obj_box", "obj_score", "obj_where", "obj_what")


def _objects(L, steps, rows, width, pp, counts, xs, ws, off=None, moved=None, **o):
    T, R, A, prob, n_in, where, what = steps, rows, width, pp, counts, xs, ws
    off = off or {}
    st = Stage()
    cap = T * R
    a = dict(prob=st.inp("presence_prob", prob), n_in=st.inp("num_objects_in", n_in), where=st.inp("where", where, off.get("where", 0)),
             what=st.inp("what", what, off.get("what", 0)), n=st.out("num_objects", (R,), dtype=torch.int32),
             count_prob=st.out("count_prob", (R,)), presence=st.out("presence", (T, R)), score=st.out("score", (T, R)),
             boxes=st.out("boxes", (T, R, 4), off.get("boxes", 0)), offsets=st.out("offsets", (R + 1,), dtype=torch.int32),
             obj_image=st.out("obj_image", (cap,), dtype=torch.int32), obj_step=st.out("obj_step", (cap,), dtype=torch.int32),
             obj_box=st.out("obj_box", (cap, 4)), obj_score=st.out("obj_score", (cap,)), obj_where=st.out("obj_where", (cap, 4)),
             obj_what=st.out("obj_what", (cap, A), off.get("obj_what", 0)))
    g = {**a, **{k: v for k, v in o.items() if k in a}}
    ptr = {k: P(g[k], 2 if k == moved else 0) for k in g}
    status = L.air_parse_objects(ptr["prob"], ptr["n_in"], ptr["where"], ptr["what"], o.get("T", T), o.get("R", R), o.get("A", A),
                                 o.get("H", RC.PS_H), o.get("W", RC.PS_W), ptr["n"], ptr["count_prob"], ptr["presence"], ptr["score"],
                                 ptr["boxes"], ptr["offsets"], *[ptr[k] for k in TABLE], stream())
    return status, st, a


def _check_table(a, n, T, R, where, what, tag):
    """offsets exact (offsets[R] too), the table the launch's own per-step outputs row by row, the rows from offsets[R] on untouched"""
    offsets = RC.exclusive_scan(n)
    same(a["offsets"], offsets, f"{tag}: offsets")
    torch.cuda.synchronize()
    for k in TABLE:                                                  # stage.untouched has no view of an output's unwritten tail
        tail = a[k][int(offsets[R]):]
        if tail.numel():
            primer = RC.INT_PRIMER if not tail.dtype.is_floating_point else None
            assert bool(torch.isnan(tail).all()) if primer is None else bool((tail == primer).all()), f"{tag}: {k} written past offsets[R]"
    want = RC.object_table(n, offsets, host(a["score"]), host(a["boxes"]), where, what)
    for k in TABLE:
        same(host(a[k])[:int(offsets[R])], want[k], f"{tag}: {k}")


def _untouched_but_tails(st):
    """Stage.untouched without the every-element-written rule for the table (its tail stays primed by design)"""
    torch.cuda.synchronize()
    for name, win, par, v, kind in st.items:
        if kind == "in":
            assert bool((bits(par) == win.parent.view(torch.int32)).all()), f"{name}: an operand has changed"
        else:
            assert RC.surroundings_intact(win, par), f"{name}: written outside its window"


@pytest.mark.parametrize("name", list(RC.PS_ROWS))
def test_Ps_objects_from_the_posterior(L, name):
    c, d = RC.PS_ROWS[name], RC.ps_data(name)
    T, R, A = c["T"], c["R"], c["A"]
    n_hat, q64, score64 = RC.count_chain64(d["prob"])
    status, st, a = _objects(L, T, R, A, d["prob"], None, d["where"], d["what"], c["off"])
    assert status == 0
    _untouched_but_tails(st)
    same(a["n"], n_hat, f"{name}: num_objects")
    same(a["presence"], (np.arange(T)[:, None] < n_hat[None, :]).astype(F32), f"{name}: presence")
    qn = q64[np.arange(R), n_hat]
    within(a["count_prob"], qn, np.abs(qn), None, "count_prob", f"{name} count_prob (one rounding)")
    within(a["score"], score64, T * np.abs(score64), None, "score", f"{name} score (T roundings)")
    box, S = RC.boxes64(d["where"], RC.PS_H, RC.PS_W)
    r = RC.worst_ratio(host(a["boxes"]), box, RC.PS_BOX_CONST * S)
    note("boxes", r, name)
    assert r <= 1.0, f"{name}: boxes, worst error / bound {r:.3g}"
    if R >= 5 and T >= 3:
        assert n_hat[:5].tolist() == [0, 0, T, 0, 0], "m_0 == m_1; all 0.5; all 1; all 0; a NaN at step 1: the terms before it decide"
        assert np.isnan(host(a["count_prob"])[4]) and np.isnan(host(a["score"])[:, 4]).all() and host(a["count_prob"])[2] == 1.0
    _check_table(a, n_hat, T, R, d["where"], d["what"], name)
    # both given: the count is the clipped input, count_prob = q(that count); the posterior outputs do not move
    n_clip = np.clip(d["n_in"], 0, T)
    status, st, b = _objects(L, T, R, A, d["prob"], d["n_in"], d["where"], d["what"], c["off"])
    assert status == 0
    _untouched_but_tails(st)
    same(b["n"], n_clip, f"{name}: the clipped input count")
    same(b["score"], a["score"], f"{name}: score with the count given")
    qc = q64[np.arange(R), n_clip]
    within(b["count_prob"], qc, np.abs(qc), None, "count_prob", f"{name} count_prob of a given count")
    _check_table(b, n_clip, T, R, d["where"], d["what"], name + " (count given)")
    # counts alone: score and count_prob are NaN
    status, st, e = _objects(L, T, R, A, None, d["n_in"], d["where"], d["what"], c["off"])
    assert status == 0
    assert np.isnan(host(e["score"])).all() and np.isnan(host(e["count_prob"])).all()
    same(e["n"], n_clip, f"{name}: counts alone")
    same(e["boxes"], a["boxes"], f"{name}: boxes")


@pytest.mark.parametrize("R", RC.PS_SCAN_R)
@pytest.mark.parametrize("full", [True, False])
def test_Ps_scan_and_scatter_over_the_passes(L, R, full):
    T, A = 32, 1
    rng = np.random.default_rng(R)
    n_in = np.full(R, T, np.int32) if full else rng.integers(0, T + 1, R).astype(np.int32)
    where, what = rng.standard_normal((T, R, 4)).astype(F32), rng.standard_normal((T, R, A)).astype(F32)
    status, st, a = _objects(L, T, R, A, None, n_in, where, what)
    assert status == 0
    _untouched_but_tails(st)
    _check_table(a, n_in, T, R, where, what, f"R = {R}")


OBJ_REFUSALS = [(k, {k: None}, E_NULL) for k in ("where", "what", "n", "count_prob", "presence", "score", "boxes", "offsets") + TABLE] + [
    ("no posterior and no counts", dict(prob=None), E_NULL), ("T=0", dict(T=0), E_SHAPE), ("T=33", dict(T=33), E_SHAPE),
    ("R=0", dict(R=0), E_SHAPE), ("A=0", dict(A=0), E_SHAPE), ("H=0", dict(H=0), E_SHAPE), ("where+4", dict(off={"where": 1}), E_ALIGN),
    ("boxes+4", dict(off={"boxes": 1}), E_ALIGN), ("what+2", dict(moved="what"), E_ALIGN)]


@pytest.mark.parametrize("tag,change,status", OBJ_REFUSALS, ids=[r[0] for r in OBJ_REFUSALS])
def test_Ps_objects_refusals(L, tag, change, status):
    c, d = RC.PS_ROWS["Ps_3x5x6"], RC.ps_data("Ps_3x5x6")
    o = {k: v for k, v in change.items() if k not in ("off", "moved")}
    got, st, a = _objects(L, c["T"], c["R"], c["A"], d["prob"], None, d["where"], d["what"], change.get("off"), change.get("moved"), **o)
    assert got == status
    st.untouched(written=False)


# ---------------------------------------------------------------------------------------------------------------
# Ps: air_parse_render
# ---------------------------------------------------------------------------------------------------------------
I8_FILL, I8_PRIMER = 57, -99
FORM_FIELDS = ("kernel", "NB", "RB", "threads", "lds_bytes", "vec4_glimpse", "items", "fixed_cap", "resident_cap")


class OwnerWin:
    """the int8 owner map: a window of I8_PRIMER in a parent of I8_FILL, `off` bytes off a 4-byte boundary"""

    def __init__(self, shape, off=0):
        self.n, self.lead = int(np.prod(shape)), 16 + off
        self.parent = torch.full((self.lead + self.n + 16,), I8_FILL, dtype=torch.int8)
        self.parent[self.lead:self.lead + self.n] = I8_PRIMER
        self.dev = self.parent.cuda()
        self.v = self.dev[self.lead:self.lead + self.n].view(shape)

    def intact(self, written=True):
        p = self.dev.cpu()
        edge = torch.cat([p[:self.lead], p[self.lead + self.n:]])
        inner = p[self.lead:self.lead + self.n]
        return bool((edge == I8_FILL).all()) and (bool((inner != I8_PRIMER).all()) if written else bool((inner == I8_PRIMER).all()))


def _render(L, name, thr=0.0, rec=True, layers=True, query_only=False, **o):
    c, d = RC.PR_ROWS[name], RC.pr_data(name)
    T, R, H, W, h, w = (c[k] for k in ("T", "R", "H", "W", "h", "w"))
    off = {**c["off"], **o.get("off", {})}
    st = Stage()
    f = RC.render_form(T, R, H, W, h, w, c["bands"], off.get("glimpse", 0))
    a = dict(glimpse=st.inp("glimpse", d["glimpse"], off.get("glimpse", 0)), where=st.inp("where", d["where"], off.get("where", 0)),
             presence=st.inp("presence", d["presence"]), obs=st.inp("obs", d["obs"]), recon=st.out("reconstruction", (R, H, W)),
             rec_parts=st.out("rec_parts", (f["NB"], R)) if rec else None, area=st.out("area", (T, R), dtype=torch.int32),
             layers=st.out("layers", (T, R, H, W)) if layers else None)
    ow = OwnerWin((R, H, W), off.get("owner", 0))
    a["owner"] = ow.v
    dims = [o.get(k, c[k]) for k in ("T", "R", "H", "W", "h", "w")] + [o.get("bands", c["bands"])]
    from attend_infer_repeat_amd import _lib
    form = _lib.AirWarpForm()
    qs = L.air_parse_render_form(P(a["glimpse"]), P(a["where"]), P(a["presence"]), P(a["obs"]), P(a["recon"]), P(a["rec_parts"]),
                                 P(a["owner"]), P(a["area"]), *dims, ctypes.byref(form))
    a["form"], a["form_status"], a["mirror"] = form.as_dict(), qs, f
    if query_only:
        return qs, st, a, ow
    status = L.air_parse_render(P(a["glimpse"]), P(a["where"]), P(a["presence"]), P(a["obs"]), float(F32(RC.PR_MULT)), float(F32(RC.PR_STD)),
                                float(thr), *dims, P(a["recon"]), P(a["rec_parts"]), P(a["owner"]), P(a["area"]), P(a["layers"]), stream())
    return status, st, a, ow


def _check_render(name, st, a, ow, thr, rec=True, layers=True):
    c, d, ref = RC.PR_ROWS[name], RC.pr_data(name), RC.pr_ref64(name)
    T, R, H, W, nref = c["T"], c["R"], c["H"], c["W"], d["nref"]
    st.untouched()
    assert ow.intact(), f"{name}: owner written outside its window, or a pixel left unwritten"
    recon, owner, area = host(a["recon"]), host(a["owner"]), host(a["area"])
    within(recon[:nref], ref["reconstruction"], ref["S_reconstruction"], WC.CONST["X"], "reconstruction", f"{name} reconstruction")
    rep = np.arange(R) % nref
    same(recon, recon[rep], f"{name}: reconstruction of the repeated images")
    same(owner, owner[rep], f"{name}: owner of the repeated images")
    same(area, area[:, rep], f"{name}: area of the repeated images")
    assert (area == np.stack([(owner == t).sum((1, 2)) for t in range(T)])).all(), f"{name}: area is the count of owner == t"
    if layers:
        lay = host(a["layers"])
        within(lay[:, :nref], ref["layers"], ref["S_layers"], WC.CONST["X"], "layers", f"{name} layers")
        same(lay, lay[:, rep], f"{name}: layers of the repeated images")
        assert (lay[d["presence"] <= 0.5] == 0).all(), f"{name}: the layer of an absent step is exactly 0"
        want, _ = RC.owner_rule(lay, d["presence"], thr)
        same(owner, want, f"{name}: owner is the rule applied to the launch's own layers")
    if rec:
        f = a["mirror"]
        parts = host(a["rec_parts"])
        for band in range(f["NB"]):
            rows = slice(band * f["RB"], min((band + 1) * f["RB"], H))
            r64, S = ref["rec_pix"][:, rows].sum((1, 2)), ref["S_rec_pix"][:, rows].sum((1, 2))
            fin = np.isfinite(r64)
            assert (np.isnan(parts[band, :nref]) == ~fin).all()
            if fin.any():
                r = float((np.abs(parts[band, :nref][fin] - r64[fin]) / WC.rec_bound(S[fin])).max())
                note("rec_parts", r, name)
                assert r <= 1.0, f"{name}: rec_parts of band {band}, worst error / bound {r:.3g}"
        same(parts, parts[:, rep], f"{name}: rec_parts of the repeated images")
    return recon, owner, area


@pytest.mark.parametrize("name", list(RC.PR_ROWS))
def test_Ps_render(L, name):
    c, d = RC.PR_ROWS[name], RC.pr_data(name)
    T, R, H, W, h, w = (c[k] for k in ("T", "R", "H", "W", "h", "w"))
    status, st, a, ow = _render(L, name)
    assert a["form_status"] == 0 and {k: a["form"][k] for k in FORM_FIELDS} == {k: a["mirror"][k] for k in FORM_FIELDS}, (a["form"], a["mirror"])
    assert status == 0
    recon, owner, area = _check_render(name, st, a, ow, 0.0)
    # the canvas is air_canvas_unroll_fwd's for the same presences, bit for bit
    st2 = Stage()
    g, wh, pr = st2.inp("glimpse", d["glimpse"]), st2.inp("where", d["where"]), st2.inp("presence", d["presence"])
    final = st2.out("final_canvas", (R, H, W))
    assert L.air_canvas_unroll_fwd(P(g), P(wh), P(pr), None, None, P(final), None, T, R, H, W, h, w, float(F32(RC.PR_MULT)), float(F32(RC.PR_STD)),
                                   stream()) == 0
    st2.untouched()
    same(recon, (F32(RC.PR_MULT) * host(final)).astype(F32), f"{name}: reconstruction against mult * the unrolled canvas")
    kind = c.get("presence")
    if kind == "101_and_absent":
        assert (recon[1] == 0).all() and (owner[1] == -1).all() and (area[:, 1] == 0).all(), "all absent: canvas exactly 0, owner -1"
        assert (owner[0] != 1).all(), "the absent middle step owns nothing"
    if c.get("twins"):
        assert not (owner[0] == 2).any() and (owner[0] == 0).any(), "two identical steps: the smaller one owns"
    if c.get("nan_glimpse"):
        assert np.isnan(recon[0]).any() and not np.isnan(recon[1]).any()
        lay = host(a["layers"])
        assert not ((owner[0] == 1) & np.isnan(lay[1, 0])).any(), "a NaN layer owns nothing"
    # mask_threshold at one pixel's top, read back from layers: that pixel is -1 (strict >)
    lay = host(a["layers"])
    _, top = RC.owner_rule(lay, d["presence"], 0.0)
    cand = np.argwhere(owner >= 0)
    assert len(cand) and (recon[:d["nref"]] != 0).any(), f"{name}: the row renders nothing (every image absent)"
    if len(cand):
        b, i, j = cand[len(cand) // 2]
        thr = float(top[b, i, j])
        status, st3, a3, ow3 = _render(L, name, thr=thr)
        assert status == 0
        _, owner3, _ = _check_render(name, st3, a3, ow3, thr)
        assert owner3[b, i, j] == -1 and (owner3 >= 0).any() or thr == float(top.max())
    # rec_parts NULL; layers NULL: the other outputs keep their bits
    status, st4, a4, ow4 = _render(L, name, rec=False, layers=False)
    assert status == 0
    st4.untouched()
    assert ow4.intact()
    same(a4["recon"], recon, f"{name}: reconstruction without rec_parts and layers")
    same(a4["owner"], owner, f"{name}: owner without rec_parts and layers")
    same(a4["area"], area, f"{name}: area without rec_parts and layers")


PR_REFUSALS = [("bands not kept", dict(bands=5), True, E_SHAPE), ("LDS carve", dict(h=60, w=60, T=32), True, -5),
               ("where+4", dict(off={"where": 1}), True, E_ALIGN), ("T=33", dict(T=33), True, E_SHAPE)]


@pytest.mark.parametrize("tag,change,rec,status", PR_REFUSALS, ids=[r[0] for r in PR_REFUSALS])
def test_Ps_render_refusals(L, tag, change, rec, status):
    got, st, a, ow = _render(L, "Pr_8x16", rec=rec, **change)
    assert got == status and a["form_status"] == status
    st.untouched(written=False)
    assert ow.intact(written=False)
    if tag == "bands not kept":                                      # without rec_parts the same call is accepted
        got, st, a, ow = _render(L, "Pr_8x16", rec=False, query_only=True, **change)
        assert got == 0 and a["form"]["NB"] == 4
