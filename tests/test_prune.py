"""GPU tests of subset pruning (attend_infer_repeat_amd/prune.py, csrc/prune_kernels.hip): air_prune_score alone against
prune.reference_score on float64 oracle layers and against the existing renderer mask by mask, air_prune_select alone against
prune.reference_select on the kernel's own fp32 inputs, a planted scene through both, air_prune_relabel, then ParsePruner behind a
SceneParser / ParticleParser / ParseRefiner: the joints against float64, the decision on the device's own joints, the read-out against
air_parse_objects / air_parse_render on the compacted rows, graph replay against eager, scoring, and the public surface.

Bars.  rec_m and J_m are the kind of number rec and log w are: test_engine.py's OUT_TOL = 1e-4 (worst element / tensor max) and
OUT_L2 = 3e-5 (relative L2).  Decisions are compared exactly: either the reference's winner is ahead by more than 2 * OUT_TOL * max|J|
(asserted in the test), or the rule is applied to the device's own float64 joints."""
import dataclasses
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from oracle import air_oracle as O
from test_engine import OUT_L2, OUT_TOL, check_tensor
from test_parse import MASK_THRESHOLD, SENTINEL_F, SENTINEL_I, _mnist_air, _train_state, e2e_case, engine_config, make_parser, \
    run_objects, run_render
from test_refine import mixed_counts, same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
dev_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. / 2. air_prune_score alone ------------------------------------------------------------------------------------------------
SCORE_CASES = {"5x6_T3_B2": ((5, 6), (3, 4), 3, 2), "7x5_T1_B1": ((7, 5), (3, 3), 1, 1), "12x10_T6_B2": ((12, 10), (4, 5), 6, 2),
               "28x36_T5_B3": ((28, 36), (9, 12), 5, 3), "50x50_T3_B1": ((50, 50), (20, 20), 3, 1)}
MULT, STD = 0.5, 0.3


def score_case(name):
    (H, W), (h, w), T, B = SCORE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    glimpse = rng.normal(size=(T, B, h, w)).astype(np.float32)
    where = np.empty((T, B, 4), np.float32)
    where[..., 0::2] = rng.uniform(0.3, 1.2, (T, B, 2)) * rng.choice([-1.0, 1.0], (T, B, 2), p=[0.3, 0.7])
    where[..., 1::2] = rng.normal(size=(T, B, 2)) * 0.4
    where[0, 0, 1] = 0.9                                           # partly outside the canvas
    where[T - 1, B - 1, 3] = 5.0                                   # wholly outside
    n = np.array([T, 0, T // 2, 1][:B]) if B > 1 else np.array([T])
    presence = (np.arange(T)[:, None] < n[None, :]).astype(np.float32)
    obs = rng.uniform(size=(B, H, W)).astype(np.float32)
    return dict(glimpse=glimpse, where=where, presence=presence, obs=obs, n=n, img=(H, W), crop=(h, w), T=T, B=B)


def run_score(case, all_candidates, n_bands=None, presence=None):
    """air_prune_score alone (current stream); rec_sub starts as a sentinel fill.  Returns (rec_sub [n_bands, B, 2^T], status)"""
    from attend_infer_repeat_amd import hip as Hh
    (H, W), (h, w), T, B = case["img"], case["crop"], case["T"], case["B"]
    L, p = Hh.lib(), Hh._p
    nb = int(L.air_canvas_unroll_bands(B, H)) if n_bands is None else n_bands
    d = {k: dev_t(case[k]) for k in ("glimpse", "where", "obs")}
    d["presence"] = dev_t(case["presence"] if presence is None else presence)
    rec_sub = torch.full((nb, B, 1 << T), SENTINEL_F).cuda()
    st = L.air_prune_score(p(d["glimpse"]), p(d["where"]), p(d["presence"]), p(d["obs"]), MULT, STD, int(all_candidates), T, B, H, W,
                           h, w, nb, p(rec_sub), Hh._stream())
    torch.cuda.synchronize()
    return rec_sub, st


def band_sum(rec_sub):
    rec = rec_sub[0].clone()
    for k in range(1, rec_sub.shape[0]):
        rec = rec + rec_sub[k]
    return rec


def f64_layers(case):
    g, w = torch.from_numpy(case["glimpse"]).double(), torch.from_numpy(case["where"]).double()
    return torch.stack([O.st_write(g[t], w[t], case["img"]) for t in range(case["T"])], 0).numpy()


@pytest.mark.parametrize("all_candidates", [0, 1])
@pytest.mark.parametrize("name", list(SCORE_CASES))
def test_score_matches_reference_score(gpu_device, name, all_candidates):
    from attend_infer_repeat_amd import prune
    case = score_case(name)
    T, B = case["T"], case["B"]
    got, st = run_score(case, all_candidates)
    assert st == 0
    if name.startswith("50x50"):
        assert got.shape[0] > 1 and case["img"][0] % got.shape[0] != 0      # several bands, a short last one
    ref = prune.reference_score(case["glimpse"], case["where"], case["presence"], case["obs"], MULT, STD, all_candidates,
                                layers=f64_layers(case))
    own = prune.reference_score(case["glimpse"], case["where"], case["presence"], case["obs"], MULT, STD, all_candidates)
    assert np.allclose(own, ref, rtol=1e-12, atol=1e-9, equal_nan=True)    # the module's own inverse warp is the oracle's
    c = np.full(B, T) if all_candidates else case["n"]
    live = np.arange(1 << T)[None, :] < (1 << c)[:, None]
    assert np.array_equal(np.isnan(ref), ~live) and live[:, 0].all()
    g = got.cpu().numpy()
    assert (g[:, ~live] == SENTINEL_F).all() and not (g[:, live] == SENTINEL_F).any()      # only the candidates' masks are written
    total = band_sum(got).cpu().numpy()
    check_tensor("prune_score", "%s_all%d" % (name, all_candidates), "out", "rec_sub", torch.from_numpy(total[live]),
                 torch.from_numpy(ref[live]), OUT_TOL, OUT_L2)
    again, _ = run_score(case, all_candidates)
    assert torch.equal(again, got)                                 # the same bits run to run


@pytest.mark.parametrize("name", list(SCORE_CASES))
def test_score_matches_the_renderer_mask_by_mask(gpu_device, name):
    """Worst observed on an MI355X (worst element / tensor max): 0 at 5x6, 7x5 and 12x10 (one wave's worth of pixels per band: the same
    order of adds), 1.13e-7 at 28x36 / T = 5 and 1.07e-7 at 50x50 / 8 bands (bar 1e-4)."""
    case = score_case(name)
    T, B = case["T"], case["B"]
    got, st = run_score(case, 1)
    assert st == 0
    total = band_sum(got).cpu().double()
    d = {k: dev_t(case[k]) for k in ("glimpse", "where", "obs")}
    ref = torch.empty(B, 1 << T, dtype=torch.float64)
    for m in range(1 << T):
        pres = torch.tensor([[float((m >> t) & 1)] * B for t in range(T)]).cuda()
        r = run_render(d["glimpse"], d["where"], pres, d["obs"], MULT, STD, case["img"], case["crop"], layers=False)
        assert r["n_bands"] == got.shape[0]
        ref[:, m] = r["rec"].cpu().double()
    err = ((total - ref).abs().max() / ref.abs().max()).item()
    print("prune_score %s against air_parse_render over %d masks: worst / max %.3g" % (name, 1 << T, err))
    assert err < OUT_TOL
    # "present": the same numbers wherever an entry is written
    pres_mode, _ = run_score(case, 0)
    live = torch.from_numpy(np.arange(1 << T)[None, :] < (1 << case["n"])[:, None])
    assert torch.equal(band_sum(pres_mode).cpu()[live], band_sum(got).cpu()[live])


def test_score_argument_checks(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = score_case("5x6_T3_B2")
    nb = int(Hh.lib().air_canvas_unroll_bands(2, 5))
    got, st = run_score(case, 0, n_bands=nb + 1)                   # not the library's banding
    assert st == -2 and (got == SENTINEL_F).all()
    for T in (0, 7):
        bad = dict(case, T=T)
        bad["glimpse"] = np.zeros((max(T, 1), 2, 3, 4), np.float32)
        got, st = run_score(bad, 0, n_bands=nb)
        assert st == -2 and (got == SENTINEL_F).all()
    # where off the 16-byte grid
    L, p = Hh.lib(), Hh._p
    d = {k: dev_t(case[k]) for k in ("glimpse", "presence", "obs")}
    wh = torch.zeros(3 * 2 * 4 + 4).cuda()
    out = torch.full((nb, 2, 8), SENTINEL_F).cuda()
    st = L.air_prune_score(p(d["glimpse"]), p(wh[1:]), p(d["presence"]), p(d["obs"]), MULT, STD, 0, 3, 2, 5, 6, 3, 4, nb, p(out), Hh._stream())
    assert st == -3
    st = L.air_prune_score(p(d["glimpse"]), None, p(d["presence"]), p(d["obs"]), MULT, STD, 0, 3, 2, 5, 6, 3, 4, nb, p(out), Hh._stream())
    assert st == -1
    # a carve above the LDS the kernel may use: AIR_E_UNSUPPORTED before any launch (nothing is read)
    st = L.air_prune_score(p(d["glimpse"]), p(wh), p(d["presence"]), p(d["obs"]), MULT, STD, 0, 6, 1, 8, 8, 100, 100, 8, p(out), Hh._stream())
    assert st == -5
    torch.cuda.synchronize()
    assert (out == SENTINEL_F).all()


# ---- 3. air_prune_select alone ------------------------------------------------------------------------------------------------------
SELECT_OUT = dict(J_sub=("f8", lambda T, B, A, G: (B, 1 << T)), best_mask=("i4", lambda T, B, A, G: (B,)),
                  num_objects_out=("i4", lambda T, B, A, G: (B,)), kept_step=("i4", lambda T, B, A, G: (T, B)),
                  objective=("f8", lambda T, B, A, G: (B,)), objective_start=("f8", lambda T, B, A, G: (B,)),
                  evidence=("f8", lambda T, B, A, G: (T, B)), what_out=("f4", lambda T, B, A, G: (T, B, A)),
                  where_out=("f4", lambda T, B, A, G: (T, B, 4)), glimpse_out=("f4", lambda T, B, A, G: (T, B, G)),
                  score_out=("f4", lambda T, B, A, G: (T, B)))
TORCH_DT = {"f8": torch.float64, "f4": torch.float32, "i4": torch.int32}


def select_case(T, B, A, G, seed, n=None, n_bands=2):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)
    if n is None:
        n = rng.integers(0, T + 1, B)
        n[0] = T
        if B > 1:
            n[1] = 0
    presence = (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(np.float32)
    return dict(what=r(T, B, A), where=r(T, B, 4), glimpse=r(T, B, G), score=rng.uniform(size=(T, B)).astype(np.float32),
                presence=presence, where_loc=r(T, B, 4), rec_sub=np.zeros((n_bands, B, 1 << T), np.float32))


def run_select(case, priors, prior, normalize, all_candidates, drop=(), misalign=(), shapes=None):
    """air_prune_select alone on device copies of `case` (current stream); every output starts as a sentinel fill.  Returns (inputs and
    outputs as device tensors, the status)."""
    from attend_infer_repeat_amd import hip as Hh
    T, B, A = case["what"].shape
    G = case["glimpse"].shape[-1]
    d = {k: dev_t(v) for k, v in case.items()}
    d["prior"] = dev_t(np.asarray(prior, np.float64))
    for k in ("where", "where_loc"):
        d[k] = torch.cat([d[k].reshape(-1), torch.zeros(4).cuda()])                      # room to shift the pointer by one float
    for k, (dt, shape) in SELECT_OUT.items():
        s = shape(T, B, A, G)
        numel = int(np.prod(s)) + (4 if k == "where_out" else 0)
        d[k] = torch.full((numel,), SENTINEL_I if dt == "i4" else SENTINEL_F, dtype=TORCH_DT[dt]).cuda()
    before = {k: v.clone() for k, v in d.items()}
    ptr = {k: (None if k in drop else Hh._p(v.reshape(-1)[1:] if k in misalign else v)) for k, v in d.items()}
    pl = [NAN if v is None else float(v) for v in priors]
    t, b, a, g = shapes or (T, B, A, G)
    st = Hh.lib().air_prune_select(ptr["what"], ptr["where"], ptr["glimpse"], ptr["score"], ptr["presence"], ptr["where_loc"], *pl,
                                   ptr["prior"], int(normalize), int(all_candidates), ptr["rec_sub"], case["rec_sub"].shape[0], t, b, a, g,
                                   ptr["J_sub"], ptr["best_mask"], ptr["num_objects_out"], ptr["kept_step"], ptr["objective"],
                                   ptr["objective_start"], ptr["evidence"], ptr["what_out"], ptr["where_out"], ptr["glimpse_out"],
                                   ptr["score_out"], Hh._stream())
    torch.cuda.synchronize()
    if st != 0:
        for k in d:
            assert same_bits(d[k], before[k]), k                   # a refused call writes nothing
        return d, st
    out = dict(d)
    for k, (dt, shape) in SELECT_OUT.items():
        s = shape(T, B, A, G)
        out[k] = d[k][:int(np.prod(s))].reshape(s)
    return out, st


def craft_gaps(case, priors, prior, normalize, all_candidates, seed, gap=4.0):
    """rec_sub such that the joints of every image are a random permutation of 0, -gap, -2 gap, ...: the winner is ahead by `gap`"""
    from attend_infer_repeat_amd import prune
    T, B, _ = case["what"].shape
    base = prune.reference_select(**case, priors=priors, prior=prior, normalize_prior=normalize, all_candidates=True)["J_sub"]
    rng = np.random.default_rng(seed)
    target = np.stack([-gap * rng.permutation(1 << T) for _ in range(B)], 0).astype(np.float64)
    rec = base - target                                            # J = -rec + (latent terms + log pi) = target
    nb = case["rec_sub"].shape[0]
    case = dict(case)
    case["rec_sub"] = np.stack([(rec / nb).astype(np.float32)] * nb, 0)
    return case


def check_select(got, ref, case, all_candidates, label):
    T, B, A = case["what"].shape
    n = ref["n"]
    c = np.full(B, T) if all_candidates else n
    live = np.arange(1 << T)[None, :] < (1 << c)[:, None]
    J = got["J_sub"].cpu().numpy()
    assert np.array_equal(np.isnan(J), ~live)                      # NaN beyond 2^c, numbers below
    check_tensor("prune_select", label, "out", "J_sub", torch.from_numpy(J[live]), torch.from_numpy(ref["J_sub"][live]), OUT_TOL, OUT_L2)
    ev, ev_ref = got["evidence"].cpu().numpy(), ref["evidence"]
    cand = np.arange(T)[:, None] < c[None, :]
    assert np.array_equal(np.isnan(ev), ~cand)
    if cand.any():
        check_tensor("prune_select", label, "out", "evidence", torch.from_numpy(ev[cand]), torch.from_numpy(ev_ref[cand]), OUT_TOL, OUT_L2)
    # the winner is ahead by more than the bar can move it: no image is excluded
    Jr = np.where(live, ref["J_sub"], -np.inf)
    top2 = np.sort(Jr, axis=1)[:, ::-1][:, :2] if Jr.shape[1] > 1 else None
    bar = 2 * OUT_TOL * np.abs(ref["J_sub"][live]).max()
    if top2 is not None:
        assert ((top2[:, 0] - top2[:, 1] > bar) | (live.sum(1) == 1)).all()
    assert np.array_equal(got["best_mask"].cpu().numpy(), ref["best_mask"])
    assert np.array_equal(got["num_objects_out"].cpu().numpy(), ref["num_objects"])
    assert np.array_equal(got["kept_step"].cpu().numpy(), ref["kept_step"])
    rows = np.arange(B)
    assert np.array_equal(got["objective"].cpu().numpy(), J[rows, ref["best_mask"]])
    assert np.array_equal(got["objective_start"].cpu().numpy(), J[rows, (1 << n) - 1])
    for k in ("what", "where", "glimpse", "score"):
        assert np.array_equal(got[k + "_out"].cpu().numpy(), ref[k]), k       # bit copies (the reference gathers the fp32 inputs)


@pytest.mark.parametrize("all_candidates", [0, 1])
@pytest.mark.parametrize("shift_loc", [0.25, None])
@pytest.mark.parametrize("A,G", [(50, 400), (7, 9), (12, 16)])      # 8-byte / 4-byte / 16-byte loads of `what`; both copy paths
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [1, 3, 6])
def test_select_matches_reference_select(gpu_device, T, B, A, G, shift_loc, all_candidates):
    from attend_infer_repeat_amd import prune
    priors = (0.1, 1.5, 1.0, 0.5, shift_loc, 2.0)
    prior = np.random.default_rng(T).uniform(0.1, 1.0, T + 1)
    for normalize in (0, 1):
        case = craft_gaps(select_case(T, B, A, G, seed=100 * T + 10 * B + A), priors, prior, normalize, all_candidates, seed=B + normalize)
        ref = prune.reference_select(**case, priors=priors, prior=prior, normalize_prior=normalize, all_candidates=all_candidates)
        got, st = run_select(case, priors, prior, normalize, all_candidates)
        assert st == 0
        check_select(got, ref, case, all_candidates,
                     "T%d_B%d_A%d_G%d_%s_all%d_norm%d" % (T, B, A, G, "given" if shift_loc is not None else "centred", all_candidates,
                                                          normalize))
    if B == 5 and not all_candidates:
        assert (ref["best_mask"] >> ref["n"] == 0).all()           # "present" never keeps a bit at or above n


def test_select_ties_nan_and_infinities(gpu_device):
    """T = 2, both steps with the same latents: masks 1 and 2 have the same joint bit for bit whenever their rec entries are equal"""
    from attend_infer_repeat_amd import prune
    T, B, A, G = 2, 6, 8, 12
    case = select_case(T, B, A, G, seed=3, n=[1, 0, 1, 1, 2, 1], n_bands=1)
    for k in ("what", "where", "glimpse", "where_loc"):
        case[k][1] = case[k][0]
    inf = np.inf
    case["rec_sub"][0] = np.array([[50, 10, 10, 50],               # n = 1: masks 1 (= m0) and 2 tie at the top: m0 stays
                                   [50, 10, 10, 50],               # n = 0: the same tie, m0 = 0 loses: mask 2 is visited before mask 1
                                   [50, 10, 5, NAN],               # a NaN never wins; mask 2 does
                                   [NAN, NAN, NAN, NAN],           # all NaN: m0 stays, the objective is NaN
                                   [inf, inf, 900, inf],           # -inf loses to anything finite
                                   [NAN, NAN, inf, NAN]], np.float32)         # J = -inf replaces a NaN start
    priors, prior = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0), np.ones(3)
    ref = prune.reference_select(**case, priors=priors, prior=prior, normalize_prior=1, all_candidates=1)
    assert ref["best_mask"].tolist() == [1, 2, 2, 1, 2, 2]
    got, st = run_select(case, priors, prior, 1, 1)
    assert st == 0
    J = got["J_sub"].cpu().numpy()
    assert J[0, 1] == J[0, 2] and J[1, 1] == J[1, 2]               # the ties are ties on the device
    assert got["best_mask"].cpu().tolist() == [1, 2, 2, 1, 2, 2]
    assert got["num_objects_out"].cpu().tolist() == [1, 1, 1, 1, 1, 1]
    assert np.array_equal(got["kept_step"].cpu().numpy(), ref["kept_step"])
    obj = got["objective"].cpu().numpy()
    assert math.isnan(obj[3]) and obj[5] == -inf and np.isfinite(obj[[0, 1, 2, 4]]).all()
    assert np.isnan(got["objective_start"].cpu().numpy()[[3, 5]]).all()
    for k in ("what", "where", "glimpse", "score"):
        assert np.array_equal(got[k + "_out"].cpu().numpy(), ref[k]), k


def test_select_argument_checks_return_their_code_and_write_nothing(gpu_device):
    T, B, A, G = 3, 5, 8, 12
    priors, prior = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0), np.ones(T + 1)
    case = select_case(T, B, A, G, seed=1)
    required = ["what", "where", "glimpse", "score", "presence", "prior", "rec_sub"] + list(SELECT_OUT)
    for k in required:
        assert run_select(case, priors, prior, 1, 0, drop=(k,))[1] == -1, k
    assert run_select(case, priors, prior, 1, 0, drop=("where_loc",))[1] == 0                       # not needed with a given shift loc
    assert run_select(case, (0.0, 1.0, 0.0, 1.0, None, 1.0), prior, 1, 0, drop=("where_loc",))[1] == -1
    for shapes in ((0, B, A, G), (7, B, A, G), (32, B, A, G), (T, 0, A, G), (T, B, 0, G), (T, B, A, 0), (T, -1, A, G)):
        assert run_select(case, priors, prior, 1, 0, shapes=shapes)[1] == -2, shapes
    for k in ("where", "where_loc", "where_out"):
        assert run_select(case, priors, prior, 1, 0, misalign=(k,))[1] == -3, k
    too_many = dict(case, rec_sub=np.zeros((9, B, 1 << T), np.float32))                   # more bands than the library ever makes
    assert run_select(too_many, priors, prior, 1, 0)[1] == -2


# ---- 4. a planted scene through both kernels ------------------------------------------------------------------------------------------
def test_planted_scene_drops_the_spurious_object_and_adds_the_missing_one(gpu_device):
    """obs = two blobs; three candidate steps: the two blobs and a third blob where obs is empty"""
    from attend_infer_repeat_amd import prune
    (H, W), (h, w), T, B, A = (16, 16), (4, 4), 3, 2, 6
    glimpse = np.ones((T, B, h, w), np.float32)
    where = np.zeros((T, B, 4), np.float32)
    where[..., 0::2] = 0.3
    for t, (tx, ty) in enumerate([(-0.5, -0.5), (0.5, 0.5), (0.5, -0.5)]):
        where[t, :, 1], where[t, :, 3] = tx, ty
    n = np.array([3, 1])                                           # image 0: remove under "present"; image 1: add under "all"
    presence = (np.arange(T)[:, None] < n[None, :]).astype(np.float32)
    case = dict(glimpse=glimpse, where=where, presence=presence, img=(H, W), crop=(h, w), T=T, B=B)
    layers = f64_layers(case)
    assert all(layers[t].max() > 0.9 for t in range(T))
    case["obs"] = (MULT * (layers[0] + layers[1])).astype(np.float32)
    rng = np.random.default_rng(0)
    sel = dict(what=(rng.normal(size=(T, B, A)) * 0.5).astype(np.float32), where=where, glimpse=glimpse.reshape(T, B, -1),
               score=np.full((T, B), 0.5, np.float32), presence=presence, where_loc=where)
    priors, prior = (0.0, 1.0, 0.3, 0.5, 0.0, 1.0), np.array([0.1, 0.2, 0.4, 0.3])
    for allc, expect in ((0, [0b011, 0b001]), (1, [0b011, 0b011])):
        rec_ref = prune.reference_score(glimpse, where, presence, case["obs"], MULT, STD, allc, layers=layers)
        ref = prune.reference_select(**sel, priors=priors, prior=prior, normalize_prior=1, all_candidates=allc, rec_sub=rec_ref)
        Jr = np.where(np.isnan(ref["J_sub"]), -np.inf, ref["J_sub"])
        order = np.sort(Jr, axis=1)[:, ::-1]
        bar = 2 * OUT_TOL * np.abs(ref["J_sub"][np.isfinite(ref["J_sub"])]).max()
        assert ref["best_mask"].tolist() == expect and (order[:, 0] - order[:, 1] > bar).all()      # the float64 winner, by more than the bar
        rec_sub, st = run_score(case, allc)
        assert st == 0
        got, st = run_select(dict(sel, rec_sub=rec_sub.cpu().numpy()), priors, prior, 1, allc)
        assert st == 0
        assert got["best_mask"].cpu().tolist() == expect
        assert got["num_objects_out"].cpu().tolist() == [bin(m).count("1") for m in expect]
        ev = got["evidence"].cpu().numpy()
        assert ev[0, 0] > 0 and ev[1, 0] > 0 and ev[2, 0] < 0       # the two real objects are wanted, the third is not
        if allc:
            assert ev[1, 1] > 0 and ev[2, 1] < 0
        else:
            assert np.isnan(ev[1:, 1]).all()


# ---- 5. air_prune_relabel -------------------------------------------------------------------------------------------------------------
def test_relabel_rewrites_the_kept_rows_only(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    T, R = 4, 6
    rng = np.random.default_rng(2)
    n = np.array([0, 4, 2, 1, 3, 7])                                # (7 is clipped to T)
    nc = np.minimum(n, T)
    offsets = np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)
    src = rng.uniform(size=(T, R)).astype(np.float32)
    kept = np.stack([rng.permutation(T) for _ in range(R)], 1).astype(np.int32)
    d = dict(src=dev_t(src), kept=dev_t(kept), n=dev_t(n.astype(np.int32)), offsets=dev_t(offsets),
             score=torch.full((T, R), SENTINEL_F).cuda(), obj_score=torch.full((T * R,), SENTINEL_F).cuda(),
             obj_step=torch.full((T * R,), SENTINEL_I, dtype=torch.int32).cuda())
    p = Hh._p
    call = lambda t, r, **kw: Hh.lib().air_prune_relabel(*[kw.get(k, p(d[k])) for k in ("src", "kept", "n", "offsets")], t, r,
                                                         *[kw.get(k, p(d[k])) for k in ("score", "obj_score", "obj_step")], Hh._stream())
    assert call(0, R) == -2 and call(7, R) == -2 and call(T, 0) == -2 and call(T, R, kept=None) == -1 and call(T, R, obj_step=None) == -1
    torch.cuda.synchronize()
    assert (d["score"] == SENTINEL_F).all() and (d["obj_step"] == SENTINEL_I).all()
    assert call(T, R) == 0
    torch.cuda.synchronize()
    score, obj_score, obj_step = d["score"].cpu().numpy(), d["obj_score"].cpu().numpy(), d["obj_step"].cpu().numpy()
    want_score, want_os = np.full((T, R), SENTINEL_F, np.float32), np.full(T * R, SENTINEL_F, np.float32)
    want_step = np.full(T * R, SENTINEL_I, np.int32)
    for r in range(R):
        for j in range(nc[r]):
            want_score[j, r] = src[j, r]
            want_os[offsets[r] + j] = src[j, r]
            want_step[offsets[r] + j] = kept[j, r]
    assert np.array_equal(score, want_score) and np.array_equal(obj_score, want_os) and np.array_equal(obj_step, want_step)


# ---- 6. / 7. ParsePruner behind the providers -------------------------------------------------------------------------------------------
def make_pruner(name, candidates, particles=None, refine=None, capture=False, **cfg_kw):
    from attend_infer_repeat_amd.prune import ParsePruner
    ocfg, B, params, obs = e2e_case(name)
    if cfg_kw:
        ocfg = dataclasses.replace(ocfg, **cfg_kw)
    if particles is None:
        ps = make_parser(ocfg, B, params)
    else:
        from attend_infer_repeat_amd.particle_parse import ParticleParser
        ps = ParticleParser(engine_config(ocfg), B, particles, seed=1, mask_threshold=MASK_THRESHOLD)
        ps.load_parameters(params)
        ps.set_global_step(20000)
    base = ps
    if refine is not None:
        from attend_infer_repeat_amd.refine import ParseRefiner
        ps = ParseRefiner(base, refine, 1e-2, 1e-2)
    pr = ParsePruner(ps, candidates)
    if capture:
        base.capture()
        if ps is not base:
            ps.capture()
        pr.capture()
    return pr, ocfg, B, params, obs


def cpu(d):
    return {k: v.detach().cpu().clone() for k, v in d.items()}


def f64_reference(pr, ocfg, start, obs, J_sub=None):
    """prune.reference_score on float64 oracle layers + prune.reference_select, fed with the start parse's rows (host tensors) and the
    engine's own count table"""
    from attend_infer_repeat_amd import prune
    T, B = pr.T, pr.R
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    allc = prune.CANDIDATES[pr.candidates]
    case = dict(glimpse=start["glimpse"].reshape(T, B, h, w).numpy(), where=start["where"].numpy(), img=(H, W), T=T)
    rec = prune.reference_score(case["glimpse"], case["where"], start["presence"].numpy(), obs.reshape(B, H, W).numpy(),
                                float(ocfg.output_multiplier), float(ocfg.output_std), allc, layers=f64_layers(case))
    priors = (*ocfg.what_prior, *ocfg.where_scale_prior, *ocfg.where_shift_prior)
    return prune.reference_select(start["what"].numpy(), start["where"].numpy(), start["glimpse"].reshape(T, B, -1).numpy(),
                                  start["score"].numpy(), start["presence"].numpy(), start["where_loc"].numpy(), priors,
                                  pr.engine.prior_dev.cpu().numpy(), 1, allc, rec, J_sub=J_sub)


def check_joints_and_decision(pr, ocfg, start, obs, out, label):
    """checks a - c of every provider: the joints against float64, the decision on the device's own joints, never worse"""
    from attend_infer_repeat_amd import prune
    T, B = pr.T, pr.R
    allc = prune.CANDIDATES[pr.candidates]
    ref = f64_reference(pr, ocfg, start, obs)
    J = out["objective_subsets"].numpy()
    live = ~np.isnan(ref["J_sub"])
    assert np.array_equal(~np.isnan(J), live)
    check_tensor("prune", label, "out", "objective_subsets", torch.from_numpy(J[live]), torch.from_numpy(ref["J_sub"][live]), OUT_TOL, OUT_L2)
    n = ref["n"]
    assert np.array_equal(out["num_objects_start"].numpy(), n)
    own = f64_reference(pr, ocfg, start, obs, J_sub=J)             # the rule on the DEVICE's joints: exact, no image left out
    assert np.array_equal(out["best_mask"].numpy(), own["best_mask"])
    assert np.array_equal(out["kept_step"].numpy(), own["kept_step"])
    assert np.array_equal(out["num_objects"].numpy(), own["num_objects"])
    assert np.array_equal(out["objective"].numpy(), own["objective"], equal_nan=True)
    assert np.array_equal(out["objective_start"].numpy(), own["objective_start"], equal_nan=True)
    assert np.array_equal(out["evidence"].numpy(), own["evidence"], equal_nan=True)
    ok = np.isfinite(own["objective"]) & np.isfinite(own["objective_start"])
    assert (own["objective"][ok] >= own["objective_start"][ok]).all()
    for k in ("what", "where"):
        assert np.array_equal(out[k].numpy(), own[k]), k
    kept_rows = np.arange(T)[:, None] < own["num_objects"][None, :]        # (rows beyond n' keep air_parse_objects' positional score)
    assert np.array_equal(out["score"].numpy()[kept_rows], own["score"][kept_rows])
    assert np.array_equal(out["glimpse"].reshape(T, B, -1).numpy(), own["glimpse"])
    m0 = (1 << n) - 1
    print("prune %s: n %s -> best masks %s (changed %d of %d)" % (label, n.tolist(), [bin(m) for m in own["best_mask"]],
                                                                 int((own["best_mask"] != m0).sum()), B))
    return ref, own


@pytest.mark.parametrize("candidates", ["present", "all"])
@pytest.mark.parametrize("name", ["tiny", "t1_b5", "rect_t5", "mnist_b8"])
def test_pruner_behind_a_scene_parser(gpu_device, name, candidates):
    from attend_infer_repeat_amd import prune
    pr, ocfg, B, params, obs = make_pruner(name, candidates)
    T, (H, W), (h, w) = pr.T, ocfg.img_size, ocfg.crop_size
    counts = mixed_counts(ocfg, B)
    base = cpu(pr.parser.parse(obs.cuda(), counts))
    pr.synchronize()
    out_dev = pr.parse(obs.cuda(), counts)
    pr.synchronize()
    out = cpu(out_dev)
    assert set(out) == set(base) | {"objective", "objective_start", "objective_subsets", "best_mask", "kept_step", "evidence",
                                    "num_objects_start"}
    start = dict(base, where_loc=pr.where_loc.cpu().reshape(T, B, 4))
    label = "%s_%s" % (name, candidates)
    ref, own = check_joints_and_decision(pr, ocfg, start, obs, out, label)
    n, best = ref["n"], own["best_mask"]
    assert n.tolist() == counts.cpu().tolist()
    # the read-out: what air_parse_objects / air_parse_render give on the compacted rows, bit for bit
    hand = run_objects(out_dev["presence_prob"], out_dev["num_objects"], out_dev["where"], out_dev["what"], H, W)
    for k in ("num_objects", "count_prob", "presence", "boxes", "offsets"):
        assert same_bits(out_dev[k], hand[k]), k
    rows = int(out["offsets"][-1])
    for k in ("obj_image", "obj_box", "obj_where", "obj_what"):
        assert same_bits(out_dev[k][:rows], hand[k][:rows]), k
    kept_rows = np.arange(T)[:, None] < own["num_objects"][None, :]
    score_want = np.where(kept_rows, own["score"], hand["score"].cpu().numpy())
    assert np.array_equal(out["score"].numpy(), score_want, equal_nan=True)
    for b in range(B):
        lo, hi = int(out["offsets"][b]), int(out["offsets"][b + 1])
        assert out["obj_step"][lo:hi].tolist() == own["kept_step"][:hi - lo, b].tolist()
        assert np.array_equal(out["obj_score"][lo:hi].numpy(), own["score"][:hi - lo, b])
    rend = run_render(out_dev["glimpse"], out_dev["where"], out_dev["presence"], pr._start["obs"].view(B, H, W), float(ocfg.output_multiplier),
                      float(ocfg.output_std), (H, W), (h, w), layers=False)
    for k in ("reconstruction", "owner", "area", "rec"):
        assert same_bits(out_dev[k], rend[k]), k
    # the objective again, in float64 from the OUTPUT rows: the selected subset is their leading-ones chain
    again = dict(out, where_loc=torch.from_numpy(np.stack([start["where_loc"].numpy()[own["kept_step"][:, b], b] for b in range(B)], 1)))
    chain = f64_reference(types.SimpleNamespace(T=T, R=B, candidates="present", engine=pr.engine), ocfg, again, obs)
    Jmax = np.abs(ref["J_sub"][~np.isnan(ref["J_sub"])]).max()
    err = np.abs(chain["objective_start"] - out["objective"].numpy()).max()
    print("prune %s: objective against float64 on the output rows: %.3g of bar %.3g" % (label, err, OUT_TOL * Jmax))
    assert err <= OUT_TOL * Jmax
    # an image whose subset is the start parse returns the provider's parse, bit for bit
    same = np.nonzero(best == (1 << n) - 1)[0]
    for b in same:
        for k in base:
            v, u = out[k], base[k]
            if k in ("offsets",):
                continue
            if k.startswith("obj_"):
                assert same_bits(v[int(out["offsets"][b]):int(out["offsets"][b + 1])], u[int(base["offsets"][b]):int(base["offsets"][b + 1])]), k
            elif v.shape[0] == T and v.dim() > 1 and v.shape[1] == B:
                assert same_bits(v[:, b], u[:, b]), k
            else:
                assert same_bits(v[b], u[b]), k
    if candidates == "present":
        assert ((best >> n) == 0).all() and (own["num_objects"] <= n).all()


@pytest.mark.parametrize("name,particles,refine,cfg_kw", [
    ("rect_t5", 4, None, {}), ("mnist_b8", 4, None, dict(where_shift_prior=(None, 1.0))),
    ("tiny", None, 2, {}), ("rect_t5", None, 2, dict(where_shift_prior=(None, 1.0))), ("mnist_b8", 4, 2, dict(where_shift_prior=(None, 1.0)))])
def test_pruner_behind_the_other_providers(gpu_device, name, particles, refine, cfg_kw):
    pr, ocfg, B, params, obs = make_pruner(name, "all", particles=particles, refine=refine, **cfg_kw)
    args = () if particles is not None else (mixed_counts(ocfg, B),)
    kw = {} if particles is None else dict(sample_noise=False)
    if particles is not None:
        pr.parser.parse(obs.cuda())                                # draw noise once; the calls below keep it
    base = cpu(pr.parser.parse(obs.cuda(), *args, **kw))
    pr.synchronize()
    out = cpu(pr.parse(obs.cuda(), *args, **kw))
    pr.synchronize()
    assert "layers" not in out and set(base) - {"layers"} <= set(out)
    for k in ("presence_prob", "num_steps_posterior"):
        assert same_bits(out[k], base[k]), k
    if particles is not None:
        K = particles
        loc = pr.engine.where_loc.view(pr.T, B, K, 4)
        if cfg_kw:
            assert torch.equal(pr.where_loc, loc[:, :, 0])         # particle 0's rows, gathered in front of the launch list
    start = dict(base, where_loc=pr.where_loc.cpu().reshape(pr.T, B, 4))
    check_joints_and_decision(pr, ocfg, start, obs, out, "%s_K%s_refine%s%s" % (name, particles, refine, "_centred" if cfg_kw else ""))


# ---- 7b. a planted scene through the module: a winner that is non-empty, no prefix and not the start -------------------------------------
PLANTED_N = [3, 1, 2, 3, 0, 2, 1, 3]
PLANTED_FULL = (3, 7)                                              # images whose obs holds all three blobs: m0 = 0b111 stays


def planted_rows(ocfg, B):
    """three 20x20 blobs at scale 0.3: steps 0 and 2 are in obs, step 1 (between them in step order) is not -- except in the images
    PLANTED_FULL, which hold all three.  Host arrays: what, where, glimpse [T, B, h, w], obs [B, H, W], float64 layers"""
    T, A, (H, W), (h, w) = ocfg.max_steps, ocfg.n_appearance, ocfg.img_size, ocfg.crop_size
    rng = np.random.default_rng(5)
    glimpse = np.ones((T, B, h, w), np.float32)
    where = np.zeros((T, B, 4), np.float32)
    where[..., 0::2] = 0.3
    for t, (tx, ty) in enumerate([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5)]):
        where[t, :, 1], where[t, :, 3] = tx, ty
    what = (rng.normal(size=(T, B, A)) * 0.3).astype(np.float32)
    layers = f64_layers(dict(glimpse=glimpse, where=where, img=(H, W), T=T))
    canvas = layers[0] + layers[2]
    for b in PLANTED_FULL:
        canvas[b] = canvas[b] + layers[1][b]
    return what, where, glimpse, (float(ocfg.output_multiplier) * canvas).astype(np.float32), layers


@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("candidates", ["present", "all"])
def test_planted_scene_through_the_module(gpu_device, candidates, capture):
    """The provider's bound start buffers are overwritten with a planted scene and the state a provider would have returned for it
    (air_parse_objects with the planted counts, air_parse_render); then the pruner's own launch list runs (eagerly / as its graph)."""
    from attend_infer_repeat_amd import prune
    pr, ocfg, B, params, obs0 = make_pruner("mnist_b8", candidates, capture=capture)
    T, (H, W), (h, w) = pr.T, ocfg.img_size, ocfg.crop_size
    assert (T, B) == (3, 8)
    mult, std = float(ocfg.output_multiplier), float(ocfg.output_std)
    par, st, eng = pr.parser, pr._start, pr.engine
    first = pr.parse(obs0.cuda(), mixed_counts(ocfg, B))           # binds, checks the buffers, fills presence_prob and the count table
    pr.synchronize()
    what, where, glimpse, obs, layers = planted_rows(ocfg, B)
    n = torch.tensor(PLANTED_N, dtype=torch.int32).cuda()
    st["what"].copy_(dev_t(what)); st["where"].copy_(dev_t(where)); st["glimpse"].copy_(dev_t(glimpse).reshape(st["glimpse"].shape))
    st["obs"].copy_(dev_t(obs).reshape(st["obs"].shape))
    # the provider's read-out of those rows, by hand: what SceneParser.parse() would return for them
    prov = run_objects(st["presence_prob"], n, st["where"], st["what"], H, W)
    prov.update({k: v for k, v in run_render(st["glimpse"].view(T, B, h, w), st["where"], prov["presence"], st["obs"].view(B, H, W), mult,
                                             std, (H, W), (h, w), layers=False).items() if k in ("reconstruction", "owner", "area", "rec")})
    par.presence.copy_(prov["presence"]); par.score.copy_(prov["score"]); par.num_objects.copy_(prov["num_objects"])
    torch.cuda.synchronize()
    eng.wait_for_caller()
    eng._replay_or_run(pr._graph, pr._plan)
    eng.wait_for_engine()
    pr.synchronize()
    assert (pr._graph is not None) == capture
    out_dev = dict(first)                                          # the same buffers, now holding the planted scene's result
    out = cpu(out_dev)
    start = dict(what=torch.from_numpy(what), where=torch.from_numpy(where), glimpse=torch.from_numpy(glimpse), score=prov["score"].cpu(),
                 presence=prov["presence"].cpu(), where_loc=torch.from_numpy(where))
    label = "planted_%s_%s" % (candidates, "graph" if capture else "eager")
    obs_t = torch.from_numpy(obs)
    ref, own = check_joints_and_decision(pr, ocfg, start, obs_t, out, label)
    # the float64 winner, by more than the bar; non-empty, no prefix, not the start
    expect = {"present": [0b101, 0b001, 0b001, 0b111, 0b000, 0b001, 0b001, 0b111],
              "all": [0b101, 0b101, 0b101, 0b111, 0b101, 0b101, 0b101, 0b111]}[candidates]
    Jr = np.where(np.isnan(ref["J_sub"]), -np.inf, ref["J_sub"])
    order = np.sort(Jr, axis=1)[:, ::-1]
    bar = 2 * OUT_TOL * np.abs(ref["J_sub"][np.isfinite(ref["J_sub"])]).max()
    assert ref["best_mask"].tolist() == expect and ((order[:, 0] - order[:, 1] > bar) | (np.array(PLANTED_N) == 0) & (candidates == "present")).all()
    best, kept, n_out = out["best_mask"].numpy(), out["kept_step"].numpy(), out["num_objects"].numpy()
    assert best.tolist() == expect and n_out.tolist() == [bin(m).count("1") for m in expect]
    assert kept[:, 0].tolist() == [0, 2, 1]                        # the spurious middle step moved behind the two kept ones
    m0 = (1 << np.array(PLANTED_N)) - 1
    assert ((best != m0) & (best != 0) & (best != (1 << n_out) - 1)).sum() >= (1 if candidates == "present" else 6)
    # the compacted rows and the relabel: source rows, source scores, source steps
    src_score = prov["score"].cpu().numpy()
    hand = run_objects(out_dev["presence_prob"], out_dev["num_objects"], out_dev["where"], out_dev["what"], H, W)
    for b in range(B):
        ks = kept[:, b]
        assert np.array_equal(out["what"].numpy()[:, b], what[ks, b]) and np.array_equal(out["where"].numpy()[:, b], where[ks, b])
        assert np.array_equal(out["glimpse"].numpy()[:, b], glimpse[ks, b])
        lo, hi = int(out["offsets"][b]), int(out["offsets"][b + 1])
        assert hi - lo == n_out[b]
        assert out["obj_step"][lo:hi].tolist() == ks[:n_out[b]].tolist()
        assert np.array_equal(out["obj_score"][lo:hi].numpy(), src_score[ks[:n_out[b]], b])
        assert np.array_equal(out["score"].numpy()[:n_out[b], b], src_score[ks[:n_out[b]], b])
        assert np.array_equal(out["score"].numpy()[n_out[b]:, b], hand["score"].cpu().numpy()[n_out[b]:, b])
        assert (out["obj_image"][lo:hi] == b).all()
    assert not np.array_equal(out["score"].numpy()[:2, 0], src_score[:2, 0])           # (image 0: row 1 now holds step 2's score)
    for k in ("num_objects", "count_prob", "presence", "boxes", "offsets"):
        assert same_bits(out_dev[k], hand[k]), k
    rows = int(out["offsets"][-1])
    assert rows == int(n_out.sum()) > 0
    for k in ("obj_image", "obj_box", "obj_where", "obj_what"):
        assert same_bits(out_dev[k][:rows], hand[k][:rows]), k
    # the render of the compacted rows, bit for bit; and it explains obs where the winner is the truth
    rend = run_render(out_dev["glimpse"], out_dev["where"], out_dev["presence"], st["obs"].view(B, H, W), mult, std, (H, W), (h, w), layers=False)
    for k in ("reconstruction", "owner", "area", "rec"):
        assert same_bits(out_dev[k], rend[k]), k
    truth = [b for b in range(B) if expect[b] == (0b111 if b in PLANTED_FULL else 0b101)]
    assert len(truth) >= 3
    assert np.abs(out["reconstruction"].numpy()[truth] - obs[truth]).max() <= OUT_TOL * np.abs(obs).max()
    assert (out["area"].numpy()[:, truth][:2] > 0).all()           # both kept objects own pixels
    # the objective again, in float64 from the OUTPUT rows: the selected subset is their leading-ones chain
    again = dict(out, where_loc=out["where"])
    chain = f64_reference(types.SimpleNamespace(T=T, R=B, candidates="present", engine=eng), ocfg, again, obs_t)
    Jmax = np.abs(ref["J_sub"][~np.isnan(ref["J_sub"])]).max()
    err = np.abs(chain["objective_start"] - out["objective"].numpy()).max()
    print("prune %s: objective against float64 on the output rows: %.3g of bar %.3g" % (label, err, OUT_TOL * Jmax))
    assert err <= OUT_TOL * Jmax
    # images whose winner is the start parse, with objects: every key the provider would have returned, bit for bit
    same = [b for b in range(B) if best[b] == m0[b] and PLANTED_N[b] > 0]
    assert len(same) >= 2
    for b in same:
        for k in ("num_objects", "count_prob", "reconstruction", "rec", "owner"):
            assert same_bits(out_dev[k][b], prov[k][b]), k
        for k in ("presence", "score", "boxes", "area"):
            assert same_bits(out_dev[k][:, b], prov[k][:, b]), k
        for k in ("what", "where"):
            assert same_bits(out_dev[k][:, b], st[k].view(T, B, -1)[:, b]), k
        assert same_bits(out_dev["glimpse"][:, b], st["glimpse"].view(T, B, h, w)[:, b])
        lo, hi, plo = int(out["offsets"][b]), int(out["offsets"][b + 1]), int(prov["offsets"][b])
        for k in ("obj_image", "obj_step", "obj_box", "obj_score", "obj_where", "obj_what"):
            assert same_bits(out_dev[k][lo:hi], prov[k][plo:plo + hi - lo]), k
    if capture:
        pr.release_graphs(); par.release_graphs()


# ---- 8. graph -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,particles", [("mnist_b8", None), ("rect_t5", 4)])
def test_graph_replay_equals_eager(gpu_device, name, particles):
    eager, ocfg, B, params, _ = make_pruner(name, "all", particles=particles)
    graph = make_pruner(name, "all", particles=particles, capture=True)[0]
    assert graph._graph is not None and eager._graph is None
    kw = {} if particles is None else dict(sample_noise=False)
    args = (mixed_counts(ocfg, B),) if particles is None else ()
    noise = O.make_noise(ocfg, B * (particles or 1), seed=5)
    for pr in (eager, graph):
        if particles is not None:
            pr.engine.set_noise(noise["eps_where"].cuda(), noise["eps_what"].cuda(), noise["u_pres"].cuda())
    kept = []
    for seed in (11, 12):
        obs = O.synthetic_batch(ocfg, B, seed=seed)[0].cuda()
        a, b = eager.parse(obs, *args, **kw), graph.parse(obs, *args, **kw)
        eager.synchronize(); graph.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
        kept.append(b["objective_subsets"].clone())
    assert not same_bits(kept[0], kept[1])
    n = graph.launch_count()
    assert {k: v for k, v in n.items() if k != "parser"} == {"prune_score": 1, "prune_select": 1, "parse_objects": 1, "prune_relabel": 1,
                                                             "parse_render": 1, "rec_sum": 1}
    assert n["parser"] == graph.parser.launch_count() and len(graph._plan) == 6
    # update_config re-captures: a changed output_multiplier changes the joints, and changing it back restores the bits
    assert graph.update_config(output_multiplier=0.25) and graph._graph is not None
    c = graph.parse(obs, *args, **kw)["objective_subsets"].clone()
    assert not same_bits(c, kept[1])
    assert graph.update_config(output_multiplier=float(ocfg.output_multiplier))
    assert same_bits(graph.parse(obs, *args, **kw)["objective_subsets"], kept[1])
    graph.release_graphs(); graph.parser.release_graphs()


def test_set_global_step_moves_the_joints_by_the_change_of_log_pi(gpu_device):
    pr, ocfg, B, params, obs = make_pruner("tiny", "all")
    T = pr.T
    counts = mixed_counts(ocfg, B)
    tables, joints = [], []
    for step in (20000, 40000):
        pr.set_global_step(step)
        out = pr.parse(obs.cuda(), counts)
        pr.synchronize()
        tables.append(pr.engine.prior_dev.cpu().numpy().copy())
        joints.append(out["objective_subsets"].cpu().numpy().copy())
    assert not np.array_equal(tables[0], tables[1])                 # the count prior is annealed: the two steps differ
    logpi = [np.log(t / t.sum()) for t in tables]
    pop = np.array([bin(m).count("1") for m in range(1 << T)])
    delta = (logpi[1] - logpi[0])[pop][None, :]
    assert np.abs((joints[1] - joints[0]) - delta).max() <= 1e-9 * (1 + np.abs(joints[0]).max())


# ---- 9. scoring -----------------------------------------------------------------------------------------------------------------------
def test_scorer_bound_to_a_pruner_scores_the_pruned_parse(gpu_device):
    from attend_infer_repeat_amd.score import ParseScorer
    from test_score import annotated_batches
    pr, ocfg, B, params, _ = make_pruner("mnist_b8", "all")
    G = 2
    fake = types.SimpleNamespace(engine=pr.engine, T=pr.T, R=pr.R, **{k: torch.zeros_like(getattr(pr, k)) for k in
                                                                     ("owner", "boxes", "num_objects", "score", "presence")})
    sc, sc_hand = ParseScorer(pr, G, max_batches=4), ParseScorer(fake, G, max_batches=4)
    for i, b in enumerate(annotated_batches("mnist_b8", B, 2, seed=3)):
        out = pr.parse(torch.from_numpy(b["obs"]).cuda(), mixed_counts(ocfg, B))
        for k in ("owner", "boxes", "num_objects", "score", "presence"):
            assert out[k].data_ptr() == getattr(pr, k).data_ptr()
            getattr(fake, k).copy_(out[k])
        sc.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
        sc_hand.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
    a, h = sc.summary(), sc_hand.summary()
    assert set(a) == set(h) and a["images"] == 2 * B
    for k in a:
        assert a[k] == h[k] or (math.isnan(a[k]) and math.isnan(h[k])), k


# ---- 10. the model and the surface ----------------------------------------------------------------------------------------------------
NEW_KEYS = {"objective", "objective_start", "objective_subsets", "best_mask", "kept_step", "evidence", "num_objects_start"}


def test_pruning_on_the_model_does_not_disturb_training(gpu_device):
    B, T, A = 8, 3, 50
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    before = _train_state(air._engine)
    plain = {k: v.clone() for k, v in air.parse().items()}
    out = air.parse(prune="all")
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert out is air.parsed and set(out) - set(plain) == NEW_KEYS
    assert {k: tuple(out[k].shape) for k in NEW_KEYS} == {
        "objective": (B,), "objective_start": (B,), "objective_subsets": (B, 8), "best_mask": (B,), "kept_step": (T, B),
        "evidence": (T, B), "num_objects_start": (B,)}
    assert out["objective"].dtype == torch.float64 and out["best_mask"].dtype == torch.int32 and out["evidence"].dtype == torch.float64
    assert torch.equal(out["num_objects_start"], plain["num_objects"])
    for k in ("presence_prob", "num_steps_posterior"):
        assert torch.equal(out[k], plain[k]), k
    assert (out["objective"] >= out["objective_start"]).all() and torch.isfinite(out["reconstruction"]).all()
    pops = torch.tensor([bin(m).count("1") for m in out["best_mask"].tolist()], dtype=torch.int32).cuda()
    assert torch.equal(out["num_objects"], pops) and torch.equal(out["presence"].sum(0).int(), pops)
    removed = air.parse(prune="present")
    assert (removed["num_objects"] <= removed["num_objects_start"]).all()
    # cached per (provider, mode); prune=None is the old path, bit for bit; it composes behind particles and refine
    assert len(air._parse_pruners) == 2 and air.parse(prune="all") is air.parsed and len(air._parse_pruners) == 2
    with pytest.raises(ValueError, match="candidates"):
        air.parse(prune="some")
    again = air.parse()
    assert set(again) == set(plain) and all(torch.equal(again[k], plain[k]) for k in plain)
    both = air.parse(particles=2, refine=1, prune="all")
    assert NEW_KEYS | {"best_particle", "best_iter"} <= set(both) and both["objective"].dtype == torch.float64
    assert air._parser_for(2, "joint", 1, None, "all").parser is air._parser_for(2, "joint", 1, None)
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # the loggers against a torch recomputation
    from attend_infer_repeat_amd.evaluation import make_parse_logger
    got = make_parse_logger(air, lambda: (x, y), 2, "test", prune="all")(itr=3)
    assert set(got) == {"map_num_step_acc", "count_prob", "num_objects", "count_changed", "objects_dropped", "objects_added",
                        "objective_gain"}
    o = air.parse(x, prune="all")
    gain = o["objective"] - o["objective_start"]
    assert abs(got["objective_gain"] - gain.mean().item()) <= 1e-9 * (1 + abs(gain.mean().item()))
    assert got["count_changed"] == (o["num_objects"] != o["num_objects_start"]).double().mean().item()
    m0, best = ((1 << o["num_objects_start"].long()) - 1).tolist(), o["best_mask"].tolist()
    assert got["objects_dropped"] == sum(bin(a & ~b).count("1") for a, b in zip(m0, best)) / B
    assert got["objects_added"] == sum(bin(b & ~a).count("1") for a, b in zip(m0, best)) / B
    assert abs((got["objects_added"] - got["objects_dropped"]) - (o["num_objects"] - o["num_objects_start"]).double().mean().item()) < 1e-12
    got_p = make_parse_logger(air, lambda: (x, y), 1, "test", particles=2, refine=1, prune="present")(itr=3)
    assert {"count_changed", "objects_dropped", "objects_added", "objective_gain", "prune_objective_gain", "refine_moved",
            "best_particle_moved"} <= set(got_p)
    assert got_p["objects_added"] == 0.0
    # refinement and pruning together (deterministic without particles): each gain under its own key
    got_rp = make_parse_logger(air, lambda: (x, y), 1, "test", refine=2, prune="all")(itr=3)
    o = air.parse(x, refine=2, prune="all")
    g_r = torch.nan_to_num(o["refine_objective"] - o["refine_objective_start"].double(), nan=0.0, posinf=0.0, neginf=0.0).mean().item()
    g_p = torch.nan_to_num(o["objective"] - o["objective_start"], nan=0.0, posinf=0.0, neginf=0.0).mean().item()
    assert abs(got_rp["objective_gain"] - g_r) <= 1e-9 * (1 + abs(g_r)) and abs(got_rp["prune_objective_gain"] - g_p) <= 1e-9 * (1 + abs(g_p))
    plain_r = air.parse(x, refine=2)
    assert same_bits(o["refine_objective"], plain_r["objective"]) and same_bits(o["refine_objective_start"], plain_r["objective_start"])


def test_score_parse_with_pruning_and_the_score_logger(gpu_device):
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.evaluation import make_parse_score_logger
    from attend_infer_repeat_amd.score import ParseScorer
    B = 8
    air, ts, x, y = _mnist_air(B)
    d = procedural_multi_mnist(B, seed=3, n_templates=200, return_annotations=True)
    data = dict(imgs=d["imgs"].astype(np.float32) / 255.0, instances=d["instances"], boxes=d["boxes"])
    air.score_parse(torch.from_numpy(data["imgs"]).cuda(), data["instances"], data["boxes"], accumulate=False, prune="all")
    sc = air.parse_scorer(2, prune="all")
    assert sc.parser is air._parser_for(None, "joint", None, None, "all") and sc.parser.candidates == "all"
    s = sc.summary()
    assert s["images"] == B
    pr = sc.parser
    fake = types.SimpleNamespace(engine=pr.engine, T=pr.T, R=pr.R, **{k: getattr(pr, k).clone() for k in
                                                                     ("owner", "boxes", "num_objects", "score", "presence")})
    hand = ParseScorer(fake, 2)
    hand.score(data["instances"], data["boxes"], accumulate=False)
    h = hand.summary()
    for k in s:
        assert s[k] == h[k] or (math.isnan(s[k]) and math.isnan(h[k])), k
    got = make_parse_score_logger(air, data, 1, "test", prune="all")(itr=1)
    assert {"count_changed", "objects_dropped", "objects_added", "objective_gain", "count_acc", "map", "fg_ari"} <= set(got)


def test_training_script_parse_prune_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--parse-eval",
                            "--parse-prune", "all"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse+prune(all) ") == 2
    for l in rec:
        assert l["prune"] == "all" and 0.0 <= l["count_changed"] <= 1.0 and l["objective_gain"] >= 0.0
        assert l["objects_dropped"] >= 0.0 and l["objects_added"] >= 0.0
    with pytest.raises(SystemExit):
        multi_mnist.main(["--parse-prune", "some"])
