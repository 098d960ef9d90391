"""Host checks of tests/warp_cases.py (no GPU): every row of the case table against the library's host-only form queries
(air_st_read_form, air_st_read_bwd_form, air_canvas_fwd_form, air_canvas_bwd_form, air_canvas_fwd_bwd_form) under the row's own
environment switches; a row for every kernel instantiation, staging flag and workgroup size the launch rules can reach; the
off-boundary property of every `where` row, the redraw cap, the planted rows' touched-column and candidate counts; the analytic float64
gradients (whose summands give S) against float64 autograd; the float32 restatement of every comparison within RESTATEMENT_SHARE of
its bound; every planted defect at least DEFECT_MARGIN bounds away from the float64 reference.

The defects, applied to the analytic float64 backward of the rows they apply to:
  drop5      the fifth touched canvas column left out of the middle glimpse column's range (rows with the planted `touch5` transform)
  neighbour  unit 0 takes every x weight from the neighbouring canvas column's entry
  presence   presence ignored (taken as 1) at the first unit with a random transform whose presence is not 1
  border     the zero border of the staged glimpse holds 1.0
  no_s2      dwhere's scale components without the 1/s^2 of the chain
  slab       (fused launch, n_split > 1) the dwhere slab of the last split's rows left out of the sum
  mult       dcanvas formed without its leading `mult`
Every value here is a sum of random-signed terms (the glimpse, dcanvas), so every defect -- those that scale an element by a known
factor too -- changes an element by a random amount relative to S, which can be small at single elements whatever the bound: under the
GEMM group's criterion for such defects each must exceed the bound DEFECT_MARGIN x at the median touched element.  An absent step whose
presence is ignored writes non-zero values where the bound is exactly zero."""
import functools

import numpy as np
import pytest
import torch

import warp_cases as WC

NAMES = list(WC.CASES)
RUN = [n for n in NAMES if "refused" not in WC.CASES[n]["form"]]
SWITCHES = ("AIR_CANVAS_BWD_IMG", "AIR_CANVAS_GS_THREADS", "AIR_CANVAS_IMG_MIN_UNITS")


def _query(case, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    return WC.query(case, WC.host_addr(case))


@pytest.mark.parametrize("name", NAMES)
def test_every_row_names_the_form_the_library_picks(name, monkeypatch):
    case = WC.CASES[name]
    st, form = _query(case, monkeypatch)
    if "refused" in case["form"]:
        assert st == case["form"]["refused"]
        return
    assert st == 0
    assert {k: form[k] for k in case["form"]} == case["form"]
    assert form["lds_bytes"] <= 160 * 1024 and form["threads"] % 64 == 0 and form["items"] > 0


def test_queries_follow_the_switches_and_the_alignment(monkeypatch):
    """the per-call switches are read inside the form functions, and only an operand's alignment and NULL-ness enter"""
    from attend_infer_repeat_amd import hip
    A = WC.Win.BASE
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    args = (3, 700, 7, 5, 2, 4)
    assert hip.canvas_bwd_form(A, A, None, A, A, A, A, *args)[1]["IM"] == 1
    monkeypatch.setenv("AIR_CANVAS_BWD_IMG", "0")
    assert hip.canvas_bwd_form(A, A, None, A, A, A, A, *args)[1]["IM"] == 0
    monkeypatch.delenv("AIR_CANVAS_BWD_IMG")
    monkeypatch.setenv("AIR_CANVAS_IMG_MIN_UNITS", "5000")
    assert hip.canvas_bwd_form(A, A, None, A, A, A, A, *args)[1]["IM"] == 0
    monkeypatch.delenv("AIR_CANVAS_IMG_MIN_UNITS")
    for thr in (128, 256, 512, 1024, 96):
        monkeypatch.setenv("AIR_CANVAS_GS_THREADS", str(thr))
        want = thr if thr != 96 else 256
        assert hip.canvas_bwd_form(A, A, None, A, A, A, A, *args)[1]["threads"] == want
    monkeypatch.delenv("AIR_CANVAS_GS_THREADS")
    f0 = hip.st_read_form(A, A, A, 6, 3, 8, 8, 4, 4)[1]
    assert f0 == hip.st_read_form(A + 4096, A + 160, A + 16, 6, 3, 8, 8, 4, 4)[1] and f0["VEC"] == 1
    for shift in (4, 8, 12):
        assert hip.st_read_form(A, A, A + shift, 6, 3, 8, 8, 4, 4)[1]["VEC"] == 0
        assert hip.st_read_form(A, A + shift, A, 6, 3, 8, 8, 4, 4)[1]["kernel"] == "read_fwd"
        assert hip.canvas_fwd_bwd_form(A, A, A + shift, A, A, A, 1, A, A, 1, 2, 3, 12, 10, 4, 4)[1]["vec4_canvas"] == 0
    assert hip.canvas_fwd_bwd_form(A, A, A, A, A, A, 1, A, A, 1, 2, 3, 12, 10, 4, 4)[1]["vec4_canvas"] == 1
    # the fused launch's query and air_canvas_unroll_fwd_bwd_fits are the same rule
    lib = hip.lib()
    for nb, ns, T, B in ((1, 2, 2, 1024), (1, 2, 2, 1025), (4, 1, 1, 1024), (4, 1, 1, 1025), (5, 1, 2, 3), (1, 5, 2, 3), (1, 4, 2, 3)):
        st, _ = hip.canvas_fwd_bwd_form(A, A, A, A, A, A, nb, A, A, ns, T, B, 7, 5, 2, 4)
        assert (st == 0) == bool(lib.air_canvas_unroll_fwd_bwd_fits(nb, ns, T, B, 7, 5, 2, 4))


def test_every_reachable_form_has_a_row(monkeypatch):
    named = set()
    for name in RUN:
        st, form = _query(WC.CASES[name], monkeypatch)
        assert st == 0
        named |= WC.form_members(form)
    missing = [m for m in WC.REACHABLE if m not in named]
    assert not missing, missing
    kernels = [m for m in WC.REACHABLE if len(m) <= 3 and all(not isinstance(x, str) or i == 0 for i, x in enumerate(m))]
    assert len(kernels) == 1 + 4 + 1 + 1 + 3 + 2


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _kind_dims(case):
    return ("read" if case["group"] in "VW" else "write",) + tuple(case["dims"][2:])


@pytest.mark.parametrize("name", RUN)
def test_every_where_row_is_off_the_cell_boundaries(name):
    case, d = WC.CASES[name], WC.data(name)
    if case.get("identity"):
        assert (d["where_ref"].reshape(-1, 4) == np.array([1, 0, 1, 0], np.float32)).all() and case["dims"][2:4] == case["dims"][4:6]
        return
    kind, H, W, h, w = _kind_dims(case)
    rows = d["where_ref"].reshape(-1, 4)
    strict, plain = WC.boundary_distance(rows, kind, H, W, h, w)
    assert (strict > 0).all() and (plain > 0).all()
    # the device operand repeats exactly these rows
    dev = d["where"].v.numpy().reshape(d["where_ref"].shape[0], -1, 4)
    nb = d["nb"]
    assert (dev == dev[:, np.arange(dev.shape[1]) % nb]).all() and (dev[:, :nb] == d["where_ref"]).all()


def test_at_most_a_quarter_of_the_draws_is_redrawn():
    for name in RUN:
        WC.data(name)
    assert WC.DRAWS
    for key, (draws, redraws) in WC.DRAWS.items():
        assert redraws <= WC.REDRAW_CAP * draws, (key, draws, redraws)


def test_planted_rows_have_the_counts_they_are_named_for():
    seen = set()
    for name in RUN:
        case, d = WC.CASES[name], WC.data(name)
        if case["group"] in "WYZ" and not case.get("identity"):
            assert {"mirror_x", "mirror_xy", "tiny", "scale25", "scale40", "far", "small"} <= set(d["planted"]), name
            for row, (t, b) in d["planted"].items():         # ... and the operand holds them where the table says
                assert (d["where_ref"][t, b] == WC.planted_rows(*_kind_dims(case), counts=case.get("counts", False))[row]).all(), (name, row)
        if case["group"] == "W" and not case.get("identity"):
            r, b = d["planted"]["far"]
            assert (d["S_dwhere"][r, b] == 0).all() and (d["dwhere64"][r, b] == 0).all()     # exactly zero
        if case["group"] in "YZ" and not case.get("identity"):
            t, b = d["planted"]["far"]
            assert (d["write64"][t, b] == 0).all()                                              # exactly zero
            t, b = d["planted"]["tiny"]
            assert int((d["write64"][t, b] != 0).sum()) == 1                                     # the whole glimpse inside one canvas pixel
        if not case.get("counts"):
            continue
        _, _, H, W, h, w = case["dims"]
        for row, want in (("touch4", 4), ("touch5", 5)):
            t, b = d["planted"][row]
            touched, _ = WC.touched_counts(d["where_ref"][t, b], W, w)
            assert touched.max() == want and (touched[1:-1] == want).all(), (name, row, touched)
        for row, want in (("touch4", 8), ("cand8", 8), ("cand9", 9), ("touch5", 9)):
            t, b = d["planted"][row]
            touched, cand = WC.touched_counts(d["where_ref"][t, b], W, w)
            assert cand.max() == want, (name, row, cand)
            if row == "cand8":
                assert touched.max() <= 4
        seen.add(case["group"])
    assert seen == {"Y", "Z"}


def test_operands_sit_in_nan_parents_at_the_alignment_asked_for():
    for name in RUN:
        case, d = WC.CASES[name], WC.data(name)
        for key, (shape_out) in WC.operands(case).items():
            if shape_out is None or shape_out[1] or key not in d:
                continue
            win = d[key]
            assert win.shape == shape_out[0], (name, key)
            assert bool(np.isnan(win.parent[:win.lead].numpy()).all()) and bool(np.isnan(win.parent[win.lead + win.n:].numpy()).all())
            assert not bool(np.isnan(win.v.numpy()).any())
            assert (win.addr() % 16 != 0) == (key in case["off"]), (name, key)


# ---------------------------------------------------------------------------------------------------------------
# the restatement's share of every bound, and the margins of the planted defects
# ---------------------------------------------------------------------------------------------------------------
def _share(diff, S, group):
    """worst |diff| / bound; an element with S == 0 must not differ at all"""
    diff, S = np.abs(np.asarray(diff, np.float64)).reshape(-1), np.asarray(S, np.float64).reshape(-1)
    assert (diff[S == 0] == 0).all()
    nz = S > 0
    return float((diff[nz] / WC.bound(group, S[nz])).max()) if nz.any() else 0.0


def _rec32(d):
    """the reconstruction term of the oracle's float32 canvas, summed per image in float32"""
    mult, std = np.float32(WC.MULT), np.float32(WC.STD)
    z = (d["obs_ref"] - mult * d["final32"]) / std
    cst = np.float32(0.5) * np.log(np.float32(6.283185307179586)) + np.log(std)
    return (np.float32(0.5) * z * z + cst).astype(np.float32).sum((1, 2), dtype=np.float32)


def _median_margin(delta, bnd):
    delta, bnd = np.abs(delta).reshape(-1), np.asarray(bnd).reshape(-1)
    touched = delta > 0
    assert touched.any()
    with np.errstate(divide="ignore"):
        return float(np.median(delta[touched] / bnd[touched]))


@functools.lru_cache(maxsize=None)
def _analyse(name):
    """-> (worst restatement share, {defect: margin}, worst |analytic - autograd| / (2^-24 S))"""
    case, d = WC.CASES[name], WC.data(name)
    grp = case["group"]
    if case.get("identity") or grp == "V":
        return 0.0, {}, 0.0
    if grp == "W":
        share = max(_share(d["dwhere32"] - d["dwhere64"], d["S_dwhere"], grp), _share(d["dimg32"] - d["dimg64"], d["S_dimg"], grp))
        dw, di, _, _ = WC.read_bwd64(d["gathered"], d["where_ref"].reshape(-1, 4), d["dout_ref"].reshape((-1,) + d["dout_ref"].shape[2:]))
        agree = max(_share(dw.reshape(d["dwhere64"].shape) - d["dwhere64"], d["S_dwhere"], grp),
                    _share(di.reshape(d["dimg64"].shape) - d["dimg64"], d["S_dimg"], grp)) * WC.CONST[grp]
        return share, {}, agree
    if grp == "X":
        return _share(_rec32(d).astype(np.float64) - d["rec64_pix"].sum((1, 2)), d["S_rec_pix"].sum((1, 2)), "X"), {}, 0.0
    share = 0.0
    r32 = WC.autograd_write(d, torch.float32)
    keys = ("dglimpse", "dwhere", "dpresence")
    share = max([share] + [_share(r32[k] - d[k + "64"], d["S_" + k], grp) for k in keys])
    agree = max(_share(d["an_" + k] - d[k + "64"], d["S_" + k], grp) for k in keys) * WC.CONST[grp]
    # ---- defects
    T, B, H, W, h, w = case["dims"]
    nb, K = d["nb"], T * d["nb"]
    p1 = np.ones((T, nb), np.float32) if d["pres_ref"] is None else d["pres_ref"]
    dc = np.broadcast_to(d["dc64"], (T, nb, H, W)).reshape(K, H, W)
    dcabs = np.broadcast_to(d["dcabs"], (T, nb, H, W)).reshape(K, H, W)
    glm, wh = d["glm_ref"].reshape(K, h, w), d["where_ref"].reshape(K, 4)
    run = lambda pres=p1, dc_=dc, **kw: WC.write_bwd64(glm, wh, pres.reshape(K), dc_, dcabs, H=H, W=W, **kw)
    shp = {"dglimpse": (K, h, w), "dwhere": (K, 4), "dpresence": (K,)}
    ref = {k: d["an_" + k].reshape(shp[k]) for k in keys}
    bnd = {k: WC.bound(grp, d["S_" + k].reshape(shp[k])) for k in keys}
    margins = {}
    if "touch5" in d["planted"]:
        t, b = d["planted"]["touch5"]
        k, j = t * nb + b, w // 2
        c, _ = WC.coords64(wh[k][None], "write", 0, W, w)
        f = np.floor(c[0])
        cols = np.nonzero((c[0] > -1) & (c[0] < w) & ((f == j) | (f + 1 == j)))[0]
        assert len(cols) == 5
        bad = run(drop_x=(k, cols[4], j))
        margins["drop5"] = min(_median_margin((bad["dglimpse"] - ref["dglimpse"])[k, :, j], bnd["dglimpse"][k, :, j]),
                               _median_margin((bad["dwhere"] - ref["dwhere"])[k, :2], bnd["dwhere"][k, :2]))
    bad = run(neighbour=True)
    margins["neighbour"] = min(_median_margin((bad["dglimpse"] - ref["dglimpse"])[0], bnd["dglimpse"][0]),
                               _median_margin((bad["dwhere"] - ref["dwhere"])[0, 2:], bnd["dwhere"][0, 2:]))     # (x weights enter the y sums)
    free = [(t, b) for t in range(T) for b in range(nb) if p1[t, b] != 1 and (t, b) not in d["planted"].values()]
    if free:                                                # the first unit with a random transform whose presence is not one
        t, b = free[0]
        p2 = p1.copy()
        p2[t, b] = 1.0
        k = t * nb + b
        bad = run(pres=p2)
        if p1[t, b] == 0:                               # an absent step: every element it would touch has a bound of zero
            assert np.abs(bad["dglimpse"][k]).max() > 0 and bnd["dglimpse"][k].max() == 0
            margins["presence"] = float("inf")
        else:
            margins["presence"] = min(_median_margin((bad[q] - ref[q])[k], bnd[q][k]) for q in ("dglimpse", "dwhere"))
    bad = run(border=1.0)
    margins["border"] = min(_median_margin(bad["dwhere"] - ref["dwhere"], bnd["dwhere"]),
                            _median_margin(bad["dpresence"] - ref["dpresence"], bnd["dpresence"]))
    bad = run(no_s2=True)
    margins["no_s2"] = _median_margin((bad["dwhere"] - ref["dwhere"])[:, ::2], bnd["dwhere"][:, ::2])
    if case["entry"] != "write_bwd":
        mult = float(np.float32(WC.MULT))
        margins["mult"] = min(_median_margin(ref[q] / mult - ref[q], bnd[q]) for q in ("dglimpse", "dwhere"))
    if case["entry"] == "fused" and case["n_split"] > 1:
        # the last split owns glimpse rows [i0, h): its slab holds the canvas rows whose upper tap is one of them
        i0 = (h * (case["n_split"] - 1)) // case["n_split"]
        cy, _ = WC.coords64(wh, "write", 1, H, h)
        rows = (cy > -1) & (cy < h) & (np.floor(cy) + 1 >= i0)
        bad = run(dc_=dc * (~rows)[:, :, None])
        margins["slab"] = _median_margin(bad["dwhere"] - ref["dwhere"], bnd["dwhere"])
    return share, margins, agree


def test_analytic_gradients_whose_summands_give_S_are_the_autograd_gradients():
    """(a tenth of one float32 rounding of S: the two float64 evaluations differ by their own roundings only)"""
    for name in RUN:
        assert _analyse(name)[2] <= 0.1, (name, _analyse(name)[2])


def test_float32_restatement_stays_within_its_share_of_every_bound():
    worst = {}
    for name in RUN:
        share = _analyse(name)[0]
        grp = WC.CASES[name]["group"]
        grp = "X" if grp == "V" else grp
        if share > worst.get(grp, (-1.0, ""))[0]:
            worst[grp] = (share, name)
        assert share <= WC.RESTATEMENT_SHARE, (name, share)
    for grp in sorted(worst):
        print(f"\n[warp cases] group {grp}: worst float32 restatement share of the bound {worst[grp][0]:.3g} "
              f"(ratio to 2^-24 S: {worst[grp][0] * WC.CONST[grp]:.3g}, {worst[grp][1]})")
    assert sorted(worst) == sorted(WC.CONST)


def test_every_planted_defect_clears_the_bound():
    worst = {}
    for name in RUN:
        for defect, m in _analyse(name)[1].items():
            if m < worst.get(defect, (float("inf"), ""))[0] or defect not in worst:
                worst[defect] = (m, name)
    for defect in sorted(worst):
        print(f"\n[warp cases] defect {defect}: smallest margin {worst[defect][0]:.3g} bounds ({worst[defect][1]})")
    assert set(worst) == {"drop5", "neighbour", "presence", "border", "no_s2", "slab", "mult"}
    for defect, (m, name) in worst.items():
        assert m >= WC.DEFECT_MARGIN, (defect, name, m)
