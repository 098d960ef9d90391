"""GPU parity of the spatial transformer, one launch at a time (run with -m gpu on an MI355X): the glimpse read (air_st_read_fwd,
air_st_read_bwd) and the canvas launches (air_st_write_fwd, air_canvas_unroll_fwd / _banded, air_st_write_bwd, air_canvas_unroll_bwd /
_dpresence, air_canvas_unroll_fwd_bwd) on every kernel form their launch rules can reach.  Cases, references and bounds come from
tests/warp_cases.py; tests/test_warp_cases_host.py holds every row against the launch rules on the CPU, sets the bounds' constants from
a float32 restatement and checks that the planted defects clear them.

Per case: the form the library reports for the DEVICE addresses is the row's, then one launch, status 0; every output window fully
written (each starts as NaN), the SENTINEL around it and every input parent (NaN outside its window) unchanged to the bit; the images
beyond the N_REF that have a CPU reference repeat them and must repeat their results bit for bit.  A refused row returns its status and
leaves every output NaN.
  V  bits of oracle/st_loops.c in float32.
  W  dwhere, dimg within CONST * 2^-24 * S of the same loops in float64 (identity row: of the float32 loops).
  X  per-step and final canvases: bits of the oracle's sequential accumulation; the reconstruction shares, added in band order in
     float32, within the bound of float64.
  Y  dglimpse, dwhere, dpresence within the bound of float64 autograd through oracle.air_oracle.st_write; a stored-canvas row launched
     again as the recompute form: the same bits (through the unit-major form when the row is image-major, which itself agrees with the
     image-major result within the bound and in its non-finite placement); the row whose image-major carve does not fit: the bits of the
     unit-major form launched on purpose.
  Z  forward outputs: the bits of air_canvas_unroll_fwd_banded (the reconstruction shares: of its launch with the same workgroup size,
     see the test); dglimpse: the bits of the recompute form; dwhere: slab 0 bit for bit
     the recompute form's at n_split = 1, the sum of the slabs (in order, float32) within the bound otherwise; no slab element is left
     as the NaN primer, whether or not its workgroup owns a dglimpse row.
The worst error / bound of each group is printed when the module finishes (pytest -s).

Worst error / bound on an MI355X (the float32 restatement on the CPU: 0.211 / 0.197 / 0.208 / 0.249 of the bound): W 0.211 (dimg of
W_per_image_dimg), X 0.110 (the reconstruction term of Z_limit_4096), Y 0.224 (dglimpse of Y_t9_stride), Z 0.246 (dglimpse of Z_516_items).
No kernel and no launch rule had to change.  One last-bit difference surfaced: the reconstruction shares of the fused launch against
those of the banded launch at another workgroup size (2 to 4 of 24 shares at 50 x 50 in 4 bands, one unit in the last place; see
test_Z_fused_forward_backward)."""
import ctypes

import numpy as np
import pytest
import torch

import attend_cases as AC
import warp_cases as WC
from attend_cases import print_worst

pytestmark = pytest.mark.gpu
NAMES = list(WC.CASES)
SWITCHES = ("AIR_CANVAS_BWD_IMG", "AIR_CANVAS_GS_THREADS", "AIR_CANVAS_IMG_MIN_UNITS")
MULT, STD = WC.MULT, WC.STD


@pytest.fixture(scope="module")
def hip(gpu_device):
    from attend_infer_repeat_amd import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print_worst("warp kernels", list("WXYZ"))


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    same = _bits(a) == _bits(b)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in their bits"


def within(out, ref64, S, group, what):
    """|out - ref64| <= CONST[group] * 2^-24 * S elementwise (S == 0: exactly zero); the worst ratio goes to the group's report"""
    out = out.detach().cpu().double().numpy()
    ref64, S = np.asarray(ref64, np.float64), np.asarray(S, np.float64)
    assert out.shape == ref64.shape == S.shape, f"{what}: {out.shape} {ref64.shape} {S.shape}"
    assert np.isfinite(out).all(), f"{what}: {int((~np.isfinite(out)).sum())} elements not finite (an output left unwritten?)"
    err = np.abs(out - ref64)
    assert (err[S == 0] == 0).all(), f"{what}: non-zero where the bound is zero"
    nz = S > 0
    if nz.any():
        ratio = err[nz] / WC.bound(group, S[nz])
        worst = float(ratio.max())
        if group not in AC.WORST or worst > AC.WORST[group][0]:
            AC.WORST[group] = (worst, what)
        assert worst <= 1.0, f"{what}: worst error / bound {worst:.3g}"


def repeats(t, axis, nb, what):
    """member i along `axis` carries the bits of member i % nb"""
    n = t.shape[axis]
    if n > nb:
        idx = torch.arange(n, device=t.device) % nb
        same_bits(t, t.index_select(axis, idx), what + ": images beyond the referenced ones")


class Stage:
    """a case on the device: every input window (parent uploaded whole) and every output window (NaN in a SENTINEL parent)"""

    def __init__(self, name, **override):
        self.case = dict(WC.CASES[name], **override)
        self.d = WC.data(name)
        self.ops = WC.operands(self.case)
        self.win, self.par, self.v = {}, {}, {}
        off = set(self.case["off"])
        for key, spec in self.ops.items():
            if spec is None:
                continue
            shape, is_out = spec
            if is_out:
                win = WC.out_win(shape, key in off)
            elif key in self.d and self.d[key].shape == tuple(shape):
                win = self.d[key]
            else:
                win = WC.Win(shape, key in off)
                if key == "final" and "final32" in self.d:             # the stored final canvas: the oracle's, which the forward equals bit for bit
                    B = shape[0]
                    win.v.copy_(torch.from_numpy(WC._periodic(self.d["final32"], B, 0)))
                else:
                    win.v.fill_(1.0)                                    # (a refused row: never read)
            assert win.shape == tuple(shape), (name, key, win.shape, shape)
            self.win[key] = win
            self.par[key], self.v[key] = win.cuda()

    def addr(self, key):
        return self.v[key].data_ptr() if key in self.v else None

    def p(self, key):
        return ctypes.c_void_p(self.v[key].data_ptr()) if key in self.v else None

    def launch(self, hip):
        c, p, lib = self.case, self.p, hip.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        mult, std = ctypes.c_float(MULT), ctypes.c_float(STD)
        if c["group"] in "VW":
            n_img, R, H, W, h, w = c["dims"]
            n = int(round(n_img * R))
            if c["group"] == "V":
                return lib.air_st_read_fwd(p("img"), p("where"), p("glimpse"), n, n_img, H, W, h, w, stream)
            return lib.air_st_read_bwd(p("img"), p("where"), p("dglimpse"), p("dwhere"), p("dimg"), n, n_img, H, W, h, w, stream)
        T, B, H, W, h, w = c["dims"]
        ls = ctypes.c_float(1.0 / max(B, 1))
        e = c["entry"]
        if e == "write_fwd":
            return lib.air_st_write_fwd(p("glimpse"), p("where"), p("presence"), p("canvas_in"), p("final"), B, H, W, h, w, stream)
        if e == "unroll_fwd":
            return lib.air_canvas_unroll_fwd(p("glimpse"), p("where"), p("presence"), p("obs"), p("steps"), p("final"), p("rec_parts"),
                                             T, B, H, W, h, w, mult, std, stream)
        if e == "banded":
            return lib.air_canvas_unroll_fwd_banded(p("glimpse"), p("where"), p("presence"), p("obs"), p("steps"), p("final"), p("rec_parts"),
                                                    c["n_bands"], T, B, H, W, h, w, mult, std, stream)
        if e == "write_bwd":
            return lib.air_st_write_bwd(p("glimpse"), p("where"), p("presence"), p("dcanvas"), p("dglimpse"), p("dwhere"), p("dpresence"),
                                        B, H, W, h, w, stream)
        if e == "unroll_bwd":
            return lib.air_canvas_unroll_bwd(p("glimpse"), p("where"), p("presence"), p("obs"), p("final"), p("dglimpse"), p("dwhere"),
                                             T, B, H, W, h, w, mult, std, ls, stream)
        if e == "unroll_bwd_dp":
            return lib.air_canvas_unroll_bwd_dpresence(p("glimpse"), p("where"), p("presence"), p("obs"), p("final"), p("dglimpse"),
                                                       p("dwhere"), p("dpresence"), T, B, H, W, h, w, mult, std, ls, stream)
        assert e == "fused"
        return lib.air_canvas_unroll_fwd_bwd(p("glimpse"), p("where"), p("presence"), p("obs"), p("steps"), p("final"), p("rec_parts"),
                                             c["n_bands"], p("dglimpse"), p("dwhere"), c["n_split"], T, B, H, W, h, w, mult, std, ls, stream)

    def outputs(self):
        return [k for k, spec in self.ops.items() if spec is not None and spec[1]]

    def check_untouched(self, written=True):
        """outputs fully written (or, for a refused launch, still NaN), their surroundings and every input parent intact"""
        for key, spec in self.ops.items():
            if spec is None:
                continue
            if spec[1]:
                nan = torch.isnan(self.v[key])
                assert bool((~nan).all() if written else nan.all()), f"{key}: {int(nan.sum())} of {nan.numel()} elements NaN"
                assert WC.surroundings_intact(self.win[key], self.par[key]), f"{key}: written outside its window"
            else:
                same_bits(self.par[key].cpu(), self.win[key].parent, f"input {key} changed")


def run(hip, monkeypatch, name, env=None, **override):
    """the form query on the device addresses, then the launch -> (stage, status, form)"""
    st = Stage(name, **override)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (st.case.get("env", {}) if env is None else env).items():
        monkeypatch.setenv(k, v)
    status, form = WC.query(st.case, st.addr)
    got = st.launch(hip)
    torch.cuda.synchronize()
    assert got == status, (name, got, status)
    return st, status, form


def expect_form(case, status, form):
    assert status == 0
    assert {k: form[k] for k in case["form"]} == case["form"]


@pytest.mark.parametrize("name", [n for n in NAMES if "refused" in WC.CASES[n]["form"]])
def test_refused_launches_write_nothing(hip, monkeypatch, name):
    st, status, _ = run(hip, monkeypatch, name)
    assert status == st.case["form"]["refused"]
    st.check_untouched(written=False)


@pytest.mark.parametrize("name", [n for n in NAMES if WC.CASES[n]["group"] == "V" and "refused" not in WC.CASES[n]["form"]])
def test_V_read_forward(hip, monkeypatch, name):
    st, status, form = run(hip, monkeypatch, name)
    expect_form(st.case, status, form)
    st.check_untouched()
    d = st.d
    n_img, _, H, W, h, w = st.case["dims"]
    out = st.v["glimpse"].view(d["R"], n_img, h, w)
    same_bits(out[:, :d["nb"]].cpu(), torch.from_numpy(d["out32"]), name)
    repeats(out, 1, d["nb"], name)
    if n_img > d["nb"]:
        # the referenced images launched as a small batch of their own (another form when the large one streams): the same bits
        small = Stage(name, dims=(d["nb"],) + tuple(st.case["dims"][1:]))
        for key in ("img", "where"):
            R = 1 if key == "img" else d["R"]
            src = st.v[key].view((R, n_img) + tuple(st.v[key].shape[1:]))[:, :d["nb"]]
            small.v[key].copy_(src.reshape(small.v[key].shape))
        assert small.launch(hip) == 0
        torch.cuda.synchronize()
        same_bits(small.v["glimpse"].view(d["R"], d["nb"], h, w), out[:, :d["nb"]], name + ": small batch")


@pytest.mark.parametrize("name", [n for n in NAMES if WC.CASES[n]["group"] == "W" and "refused" not in WC.CASES[n]["form"]])
def test_W_read_backward(hip, monkeypatch, name):
    st, status, form = run(hip, monkeypatch, name)
    expect_form(st.case, status, form)
    st.check_untouched()
    d = st.d
    n_img, _, H, W, h, w = st.case["dims"]
    nb, ident = d["nb"], st.case.get("identity")
    dwhere = st.v["dwhere"].view(d["R"], n_img, 4)
    within(dwhere[:, :nb], d["dwhere32"].astype(np.float64) if ident else d["dwhere64"], d["S_dwhere"], "W", name + " dwhere")
    repeats(dwhere, 1, nb, name + " dwhere")
    if "dimg" in st.v:
        within(st.v["dimg"][:nb], (d["dimg32"].astype(np.float64) if ident else d["dimg64"])[0], d["S_dimg"][0], "W", name + " dimg")
        repeats(st.v["dimg"], 0, nb, name + " dimg")


def _check_forward(st, name, group_tag="X"):
    d, c = st.d, st.case
    T, B, H, W, h, w = c["dims"]
    nb = d["nb"]
    if "steps" in st.v:
        same_bits(st.v["steps"][:, :nb].cpu(), torch.from_numpy(d["steps32"]), name + " canvas_steps")
        repeats(st.v["steps"], 1, nb, name + " canvas_steps")
    if "final" in st.v and st.ops["final"][1]:
        same_bits(st.v["final"][:nb].cpu(), torch.from_numpy(d["final32"]), name + " final_canvas")
        repeats(st.v["final"], 0, nb, name + " final_canvas")
    if "rec_parts" in st.v:
        parts = st.v["rec_parts"].cpu()
        rec = parts[0].clone()
        for q in range(1, parts.shape[0]):                    # the consumers' order: band 0 + band 1 + ..., in float32
            rec = rec + parts[q]
        within(rec[:nb], d["rec64_pix"].sum((1, 2)), d["S_rec_pix"].sum((1, 2)), "X", name + " rec")
        repeats(st.v["rec_parts"], 1, nb, name + " rec_parts")


@pytest.mark.parametrize("name", [n for n in NAMES if WC.CASES[n]["group"] == "X" and "refused" not in WC.CASES[n]["form"]])
def test_X_canvas_forward(hip, monkeypatch, name):
    st, status, form = run(hip, monkeypatch, name)
    expect_form(st.case, status, form)
    st.check_untouched()
    _check_forward(st, name)


def _ref(d, case, key):
    """float64 autograd; for an identity row (every coordinate an integer) the float32 scalar oracle"""
    return d[key + "32"].astype(np.float64) if case.get("identity") else d[key + "64"]


def _check_backward(st, name, group):
    d, c = st.d, st.case
    nb = d["nb"]
    for key, axis in (("dglimpse", 1), ("dwhere", 1), ("dpresence", 1)):
        if key not in st.v:
            continue
        within(st.v[key][:, :nb], _ref(d, c, key), d["S_" + key], group, f"{name} {key}")
        repeats(st.v[key], axis, nb, f"{name} {key}")


def _classes(t):
    return torch.isnan(t) * 3 + torch.isposinf(t) * 1 + torch.isneginf(t) * 2


@pytest.mark.parametrize("name", [n for n in NAMES if WC.CASES[n]["group"] == "Y" and "refused" not in WC.CASES[n]["form"]])
def test_Y_canvas_backward(hip, monkeypatch, name):
    st, status, form = run(hip, monkeypatch, name)
    expect_form(st.case, status, form)
    st.check_untouched()
    _check_backward(st, name, "Y")
    c = st.case
    if c["entry"] == "write_bwd" or c.get("variant") != "stored":
        return
    keys = [k for k in ("dglimpse", "dwhere", "dpresence") if k in st.v]
    env = dict(c.get("env", {}))
    unit, unit_form = st, form
    if form["IM"] or name == "Y_img_carve_falls_back":
        # the unit-major form on purpose: image-major agrees with it within the bound and in its non-finite placement; the row whose
        # image-major carve does not fit already ran it, bit for bit
        unit, s2, unit_form = run(hip, monkeypatch, name, env=dict(env, AIR_CANVAS_BWD_IMG="0"))
        assert s2 == 0 and (unit_form["RC"], unit_form["IM"]) == (0, 0)
        unit.check_untouched()
        for k in keys:
            if form["IM"]:
                assert torch.equal(_classes(unit.v[k]), _classes(st.v[k])), f"{name} {k}: non-finite placement differs"
                nb = st.d["nb"]
                S = st.d["S_" + k]
                err = (unit.v[k][:, :nb] - st.v[k][:, :nb]).abs().cpu().double().numpy()
                assert (err <= WC.bound("Y", S)).all(), f"{name} {k}: image-major against unit-major {float((err / np.maximum(WC.bound('Y', S), 1e-300)).max()):.3g} bounds"
            else:
                same_bits(unit.v[k], st.v[k], f"{name} {k}: fall-back against unit-major on purpose")
        env["AIR_CANVAS_BWD_IMG"] = "0"
    # the recompute form of the same problem: the bits of the stored-canvas (unit-major) form
    rc, s3, f3 = run(hip, monkeypatch, name, env=env, variant="recompute")
    assert s3 == 0 and f3["RC"] == 1 and f3["threads"] == unit_form["threads"]
    rc.check_untouched()
    for k in keys:
        same_bits(rc.v[k], unit.v[k], f"{name} {k}: recompute against stored canvas")


@pytest.mark.parametrize("name", [n for n in NAMES if WC.CASES[n]["group"] == "Z" and "refused" not in WC.CASES[n]["form"]])
def test_Z_fused_forward_backward(hip, monkeypatch, name):
    st, status, form = run(hip, monkeypatch, name)
    expect_form(st.case, status, form)
    st.check_untouched()
    c, d = st.case, st.d
    T, B, H, W, h, w = c["dims"]
    nb, ns = d["nb"], c["n_split"]
    _check_forward(st, name)
    # forward outputs: the bits of group X's banded launch
    fw, s2, f2 = run(hip, monkeypatch, name, entry="banded", rec=True, outs="both")
    assert s2 == 0 and (f2["NB"], f2["RB"]) == (form["NB"], form["RB"])
    for k in ("steps", "final"):
        same_bits(fw.v[k], st.v[k], f"{name} {k}: fused against air_canvas_unroll_fwd_banded")
    # A band's reconstruction share is a sum of per-thread partial sums (pixels dealt over the threads with stride blockDim) through a
    # block tree: its last bit depends on the workgroup size, and the fused launch takes the backward's (512 / 256) where the banded
    # launch of a small batch takes the pixel rule's.  It is held, bit for bit, to the group X launch of the SAME workgroup size: the
    # same images repeated up to the batch at which the forward's own rule gives that size (257 .. 512 units: 512 threads, beyond: 256).
    if f2["threads"] == form["threads"]:
        same_bits(fw.v["rec_parts"], st.v["rec_parts"], f"{name} rec_parts: fused against air_canvas_unroll_fwd_banded")
    else:
        need = 257 if form["threads"] == 512 else 513
        Bx = max(B, -(-need // form["NB"]))
        big = Stage(name, entry="banded", rec=True, outs="both", dims=(T, Bx, H, W, h, w))
        idx = torch.arange(Bx, device="cuda") % B
        for k, axis in (("glimpse", 1), ("where", 1), ("presence", 1), ("obs", 0)):
            if k in big.v:
                big.v[k].copy_(st.v[k].index_select(axis, idx))
        s4, f4 = WC.query(big.case, big.addr)
        assert s4 == 0 and (f4["threads"], f4["NB"], f4["RB"], f4["vec4_glimpse"]) == (form["threads"], form["NB"], form["RB"], form["vec4_glimpse"])
        assert big.launch(hip) == 0
        torch.cuda.synchronize()
        for k, sl in (("steps", lambda t: t[:, :B]), ("final", lambda t: t[:B]), ("rec_parts", lambda t: t[:, :B])):
            same_bits(sl(big.v[k]), st.v[k], f"{name} {k}: fused against the banded launch of the same workgroup size")
    # backward: dglimpse the bits of the recompute form; dwhere slab 0 too at n_split = 1, the slab sum within the bound otherwise
    bw, s3, f3 = run(hip, monkeypatch, name, entry="unroll_bwd", variant="recompute")
    assert s3 == 0 and f3["RC"] == 1
    same_bits(bw.v["dglimpse"], st.v["dglimpse"], f"{name} dglimpse: fused against the recompute form")
    within(st.v["dglimpse"][:, :nb], _ref(d, c, "dglimpse"), d["S_dglimpse"], "Z", name + " dglimpse")
    slabs = st.v["dwhere"]
    assert bool(torch.isfinite(slabs).all()), f"{name}: a dwhere slab element left unwritten or not finite"
    if ns == 1:
        assert f3["threads"] == form["threads"]               # (both from bwd_threads(B * T): the same reduction tree)
        same_bits(slabs[0], bw.v["dwhere"], f"{name} dwhere: slab 0 against the recompute form")
    total = slabs[0].clone()
    for q in range(1, ns):
        total = total + slabs[q]
    within(total[:, :nb], _ref(d, c, "dwhere"), d["S_dwhere"], "Z", name + " dwhere (slab sum)")
    repeats(slabs, 2, nb, name + " dwhere slabs")
    repeats(st.v["dglimpse"], 1, nb, name + " dglimpse")
