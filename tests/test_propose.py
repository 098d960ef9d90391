"""GPU tests of residual proposals (attend_infer_repeat_amd/propose.py, csrc/propose_kernels.hip): air_propose_residual alone, bit for
bit against clamp(obs - reconstruction) formed from air_parse_render's output; air_propose_pool / air_propose_source alone against
propose.reference_pool; a planted scene through pool -> air_prune_score -> air_prune_select with T := C; then ParseProposer behind a
SceneParser / ParticleParser / ParseRefiner: the joints against float64 fed with the device's own pool rows, the decision on the
device's own joints, the read-out against air_parse_objects / air_parse_render on the first T compacted rows, the round invariants, a
planted scene through the module's segments, graph replay against eager, and the public surface.

Bars.  The joints and the band shares are the kind of number rec and log w are: test_engine.py's OUT_TOL = 1e-4 (worst element / tensor
max) and OUT_L2 = 3e-5 (relative L2).  Copies and decisions are compared exactly: either the reference's winner is ahead by more than
2 * OUT_TOL * max|J| (asserted in the test), or the rule is applied to the device's own float64 joints."""
import dataclasses
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from test_engine import OUT_L2, OUT_TOL, check_tensor
from test_parse import MASK_THRESHOLD, SENTINEL_F, SENTINEL_I, _mnist_air, _train_state, e2e_case, engine_config, make_parser, \
    run_objects, run_render
from test_prune import MULT, STD, cpu, dev_t, f64_layers, run_score, run_select
from test_refine import mixed_counts, same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
PRIORS = (0.0, 1.0, 0.3, 0.5, 0.0, 1.0)


# ---- 1. air_propose_residual alone ----------------------------------------------------------------------------------------------
RES_CASES = {"9x11_T2": ((9, 11), (5, 5), 2, 3), "12x10_T3": ((12, 10), (4, 6), 3, 2), "28x36_T5": ((28, 36), (8, 8), 5, 3),
             "50x50_T3": ((50, 50), (20, 20), 3, 1), "7x5_T6": ((7, 5), (3, 3), 6, 4),
             # bands above 1024 pixels (4 per thread): the pixel walk takes a second chunk, with the prefetch of the next chunk's
             # observations and their rotation -- the path of the configs[3] shapes
             "100x100_T5": ((100, 100), (28, 28), 5, 2)}


def res_case(name):
    (H, W), (h, w), T, B = RES_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    glimpse = (3.0 * rng.normal(size=(T, B, h, w))).astype(np.float32)      # canvases well above obs in places: d < 0 occurs
    where = np.empty((T, B, 4), np.float32)
    where[..., 0::2] = rng.uniform(0.3, 1.2, (T, B, 2)) * rng.choice([-1.0, 1.0], (T, B, 2), p=[0.3, 0.7])
    where[..., 1::2] = rng.normal(size=(T, B, 2)) * 0.4
    where[0, 0, 1] = 0.9                                           # partly outside the canvas
    where[T - 1, 0, 3] = 5.0                                       # wholly outside
    n = np.array([T, 0, T // 2, 1][:B])                            # n_b = T and n_b = 0 both occur (B > 1)
    obs = rng.uniform(0.0, 2.0, size=(B, H, W)).astype(np.float32)        # above clamp_hi = 1 in places
    return dict(glimpse=glimpse, where=where, n=n, obs=obs, img=(H, W), crop=(h, w), T=T, B=B)


def chain(n, T):
    return (np.arange(T)[:, None] < np.asarray(n)[None, :]).astype(np.float32)


def run_residual(case, clamp_hi=1.0, use_counts=False, n_bands=None, parts=True, drop=(), misalign=(), shape=None):
    """air_propose_residual alone (current stream); the outputs start as sentinel fills.  Returns (res, res_parts, status)"""
    from attend_infer_repeat_amd import hip as Hh
    (H, W), (h, w), T, B = case["img"], case["crop"], case["T"], case["B"]
    L, p = Hh.lib(), Hh._p
    nb = int(L.air_canvas_unroll_bands(B, H)) if n_bands is None else n_bands
    d = {k: dev_t(case[k]) for k in ("glimpse", "obs")}
    d["where"] = torch.cat([dev_t(case["where"]).reshape(-1), torch.zeros(4).cuda()])
    d["presence"] = None if use_counts else dev_t(chain(case["n"], T))
    d["counts"] = dev_t(case["n"].astype(np.int32)) if use_counts else None
    res = torch.full((B, H, W), SENTINEL_F).cuda()
    res_parts = torch.full((nb, B), SENTINEL_F).cuda() if parts else None
    ptr = {k: (None if k in drop or v is None else p(v.reshape(-1)[1:] if k in misalign else v)) for k, v in d.items()}
    t, b, hh, ww = shape or (T, B, h, w)
    st = L.air_propose_residual(ptr["glimpse"], ptr["where"], ptr["presence"], ptr["counts"], ptr["obs"], MULT, float(clamp_hi), t, b, H,
                                W, hh, ww, nb, p(res), p(res_parts), Hh._stream())
    torch.cuda.synchronize()
    return res, res_parts, st


def residual_from_render(case, clamp_hi=1.0):
    """clamp(obs - reconstruction) in fp32 from air_parse_render's reconstruction of the same rows and presence chain"""
    d = {k: dev_t(case[k]) for k in ("glimpse", "where", "obs")}
    r = run_render(d["glimpse"], d["where"], dev_t(chain(case["n"], case["T"])), d["obs"], MULT, STD, case["img"], case["crop"], layers=False)
    diff = d["obs"] - r["reconstruction"]
    return torch.where(diff > 0, torch.clamp(diff, max=clamp_hi), torch.zeros_like(diff)), r["n_bands"]


@pytest.mark.parametrize("name", list(RES_CASES))
def test_residual_is_bit_equal_to_the_renderer(gpu_device, name):
    case = res_case(name)
    T, B = case["T"], case["B"]
    got, parts, st = run_residual(case)
    assert st == 0
    want, nb = residual_from_render(case)
    assert parts.shape[0] == nb
    H, W = case["img"]
    rb = -(-H // nb)                                               # air_canvas_unroll_bands' banding: bands of ceil(H / n_bands) rows
    if name.startswith("50x50") or name.startswith("100x100"):
        assert nb > 1 and H % nb != 0 and -(-H // rb) == nb        # several bands, a short last one
    if name.startswith("100x100"):
        assert 1024 < rb * W < 2048 and 0 < (H - (nb - 1) * rb) * W < 1024      # two chunks per full band, one in the last
    assert torch.equal(got, want)
    assert (got == 1.0).any() and (got == 0.0).any() and (got >= 0).all() and (got <= 1.0).all()      # both ends of the clamp are hit
    if B > 1:
        assert torch.equal(got[1], torch.clamp(dev_t(case["obs"])[1], max=1.0))      # n_b = 0: the clamped image itself
    # the same bits from given counts, without the band shares, and run to run
    by_counts, parts_c, st = run_residual(case, use_counts=True)
    assert st == 0 and torch.equal(by_counts, got) and torch.equal(parts_c, parts)
    plain, none, st = run_residual(case, parts=False)
    assert st == 0 and none is None and torch.equal(plain, got)
    # another clamp
    low, _, st = run_residual(case, clamp_hi=0.25)
    assert st == 0 and torch.equal(low, residual_from_render(case, 0.25)[0]) and (low == 0.25).any() and (low <= 0.25).all()
    # the residual and the band shares against float64
    ref, energy = _f64_residual(case)
    check_tensor("propose_residual", name, "out", "res", got.cpu(), torch.from_numpy(ref), OUT_TOL, OUT_L2)
    tot = parts[0].clone()
    for k in range(1, nb):
        tot = tot + parts[k]
    check_tensor("propose_residual", name, "out", "res_energy", tot.cpu(), torch.from_numpy(energy), OUT_TOL, OUT_L2)
    # ... and every band's share against the float64 sum over that band's rows
    shares = np.stack([(ref[:, k * rb:min((k + 1) * rb, H)] ** 2).reshape(B, -1).sum(1) for k in range(nb)], 0)
    assert np.allclose(shares.sum(0), energy, rtol=1e-12)
    check_tensor("propose_residual", name, "out", "res_parts", parts.cpu(), torch.from_numpy(shares), OUT_TOL, OUT_L2)


def _f64_residual(case, clamp_hi=1.0):
    """propose.reference_residual's rule on the float64 oracle layers (and a check that the module's own warp is the oracle's)"""
    from attend_infer_repeat_amd import propose
    layers = f64_layers(case)
    B = case["B"]
    canvas = np.zeros((B,) + tuple(case["img"]))
    for t in range(case["T"]):
        canvas = np.where((t < case["n"])[:, None, None], canvas + layers[t], canvas)
    d = case["obs"].astype(np.float64) - MULT * canvas
    res = np.where(d > 0, np.minimum(d, clamp_hi), 0.0)
    own, energy = propose.reference_residual(case["glimpse"], case["where"], case["n"], case["obs"], MULT, clamp_hi)
    assert np.allclose(own, res, rtol=1e-12, atol=1e-9)
    return res, energy


def test_residual_nan_in_a_glimpse_gives_zero(gpu_device):
    case = res_case("12x10_T3")
    case["glimpse"][0, 0, 1, 2] = NAN
    got, _, st = run_residual(case)
    assert st == 0 and not torch.isnan(got).any()
    want, _ = residual_from_render(case)
    assert torch.equal(got, want)
    d = {k: dev_t(case[k]) for k in ("glimpse", "where", "obs")}
    rec = run_render(d["glimpse"], d["where"], dev_t(chain(case["n"], 3)), d["obs"], MULT, STD, case["img"], case["crop"], layers=False)
    hit = torch.isnan(rec["reconstruction"])
    assert hit[0].any() and not hit[1:].any() and (got[hit] == 0).all()


def test_residual_argument_checks_return_their_code_and_write_nothing(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    case = res_case("12x10_T3")
    nb = int(Hh.lib().air_canvas_unroll_bands(2, 12))
    untouched = lambda res, parts: (res == SENTINEL_F).all() and (parts is None or (parts == SENTINEL_F).all())
    res, parts, st = run_residual(case, n_bands=nb + 1)            # not the library's banding
    assert st == -2 and untouched(res, parts)
    for shape in ((0, 2, 4, 6), (7, 2, 4, 6), (3, 0, 4, 6), (3, 2, 0, 6), (3, 2, 4, -1)):
        res, parts, st = run_residual(case, n_bands=nb, shape=shape)
        assert st == -2 and untouched(res, parts), shape
    for k in ("glimpse", "where", "obs"):
        res, parts, st = run_residual(case, drop=(k,))
        assert st == -1 and untouched(res, parts), k
    res, parts, st = run_residual(case, drop=("presence",))          # neither a chain nor counts
    assert st == -1 and untouched(res, parts)
    res, parts, st = run_residual(case, misalign=("where",))
    assert st == -3 and untouched(res, parts)
    # a carve above the LDS the kernel may use: AIR_E_UNSUPPORTED before any launch (nothing is read)
    big = dict(case, img=(8, 8), B=1, T=6)
    nb8 = int(Hh.lib().air_canvas_unroll_bands(1, 8))
    res, parts, st = run_residual(big, n_bands=nb8, shape=(6, 1, 100, 100))
    assert st == -5 and untouched(res, parts)


# ---- 2. air_propose_pool / air_propose_source alone --------------------------------------------------------------------------------
def run_pool(T, P, B, A, G, seed, n, use_counts, source_in, rnd, misalign=()):
    """air_propose_pool on random rows; the pool buffers have one sentinel row beyond C.  Returns (host inputs, device pool, status)"""
    from attend_infer_repeat_amd import hip as Hh
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)
    C = T + P
    host = dict(what=r(T, B, A), where=r(T, B, 4), glimpse=r(T, B, G), score=r(T, B), prop_what=r(T, B, A), prop_where=r(T, B, 4),
                prop_glimpse=r(T, B, G), prop_score=r(T, B), prior=rng.uniform(0.1, 1.0, T + 1))
    pad = lambda a: torch.cat([dev_t(a).reshape(-1), torch.zeros(4, dtype=dev_t(a).dtype).cuda()])      # room to shift by one float
    d = {k: pad(v) for k, v in host.items() if k != "prior"}
    d["prior"] = dev_t(host["prior"])
    d["presence"] = None if use_counts else dev_t(chain(np.clip(n, 0, T), T))
    d["counts"] = dev_t(np.asarray(n, np.int32)) if use_counts else None
    d["source_in"] = None if source_in is None else dev_t(source_in.astype(np.int32))
    ff = lambda *s: torch.full(s, SENTINEL_F).cuda()
    pool = dict(what=ff((C + 1) * B * A + 4), where=ff(C + 1, B, 4), glimpse=ff((C + 1) * B * G + 4), score=ff(C + 1, B), presence=ff(C + 1, B),
                source=torch.full((C + 1, B), SENTINEL_I, dtype=torch.int32).cuda(),
                prior=torch.full((C + 2,), SENTINEL_F, dtype=torch.float64).cuda())
    p = Hh._p
    off = lambda k, t: p(t.reshape(-1)[1:]) if k in misalign else p(t)
    st = Hh.lib().air_propose_pool(off("what", d["what"]), p(d["where"]), off("glimpse", d["glimpse"]), p(d["score"]), p(d["presence"]),
                                   p(d["counts"]), p(d["source_in"]), p(d["prop_what"]), p(d["prop_where"]), p(d["prop_glimpse"]),
                                   p(d["prop_score"]), p(d["prior"]), rnd, T, P, B, A, G, off("pool_what", pool["what"]), p(pool["where"]),
                                   off("pool_glimpse", pool["glimpse"]), p(pool["score"]), p(pool["presence"]), p(pool["source"]),
                                   p(pool["prior"]), Hh._stream())
    torch.cuda.synchronize()
    if "what" in misalign:                                         # the kernel read what the shifted pointer shows
        flat = d["what"].cpu().numpy()
        host["what"] = flat[1:1 + T * B * A].reshape(T, B, A)
    if "glimpse" in misalign:
        flat = d["glimpse"].cpu().numpy()
        host["glimpse"] = flat[1:1 + T * B * G].reshape(T, B, G)
    o = 1 if "pool_what" in misalign else 0
    pool["what"] = pool["what"][o:o + (C + 1) * B * A].reshape(C + 1, B, A)
    o = 1 if "pool_glimpse" in misalign else 0
    pool["glimpse"] = pool["glimpse"][o:o + (C + 1) * B * G].reshape(C + 1, B, G)
    return host, pool, st


@pytest.mark.parametrize("misalign", [(), ("what", "glimpse"), ("pool_what", "pool_glimpse")])
@pytest.mark.parametrize("A,G", [(8, 16), (7, 9)])                  # a multiple of 4 and not: both copy paths (and both with misaligned buffers)
@pytest.mark.parametrize("T,P,B", [(2, 1, 3), (3, 3, 5), (5, 1, 6)])
def test_pool_and_source_match_the_reference(gpu_device, T, P, B, A, G, misalign):
    from attend_infer_repeat_amd import hip as Hh, propose
    C = T + P
    rng = np.random.default_rng(T * 10 + B)
    n = rng.integers(0, T + 1, B)
    n[0], n[1] = T, 0
    for use_counts, source_in, rnd in ((False, None, 0), (True, np.stack([rng.permutation(C + 3) for _ in range(B)], 1), 2)):
        if use_counts:
            n = n.copy()
            n[-1] = T + 4                                          # clipped to T
        host, pool, st = run_pool(T, P, B, A, G, seed=A + T, n=n, use_counts=use_counts, source_in=source_in, rnd=rnd, misalign=misalign)
        assert st == 0
        ref = propose.reference_pool(host["what"], host["where"], host["glimpse"], host["score"], n, host["prop_what"], host["prop_where"],
                                     host["prop_glimpse"], host["prop_score"], host["prior"], P, round=rnd, source_in=source_in)
        for k in ("what", "where", "glimpse", "score", "presence", "source"):
            assert np.array_equal(pool[k][:C].cpu().numpy().view(np.int32), np.ascontiguousarray(ref[k]).view(np.int32)), k      # bit copies
            sentinel = SENTINEL_I if k == "source" else SENTINEL_F
            assert (pool[k][C] == sentinel).all(), k               # the row beyond C is untouched
        assert np.array_equal(pool["prior"][:C + 1].cpu().numpy(), ref["prior"]) and pool["prior"][C + 1].item() == SENTINEL_F
        # provenance behind a selection
        kept = np.stack([rng.permutation(C) for _ in range(B)], 1).astype(np.int32)
        out = torch.full((C + 1, B), SENTINEL_I, dtype=torch.int32).cuda()
        st = Hh.lib().air_propose_source(Hh._p(pool["source"]), Hh._p(dev_t(kept)), C, B, Hh._p(out), Hh._stream())
        torch.cuda.synchronize()
        assert st == 0 and np.array_equal(out[:C].cpu().numpy(), propose.reference_source(ref["source"], kept)) and (out[C] == SENTINEL_I).all()


def test_pool_and_source_argument_checks(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    L, p = Hh.lib(), Hh._p
    f = torch.zeros(6 * 2 * 8).cuda()
    i = torch.full((7, 2), SENTINEL_I, dtype=torch.int32).cuda()
    d = torch.full((8,), SENTINEL_F, dtype=torch.float64).cuda()
    out = torch.full((6 * 2 * 8,), SENTINEL_F).cuda()
    call = lambda T, P, R, A, G, **kw: L.air_propose_pool(p(f), p(f), p(f), p(f), kw.get("presence", p(f)), None, None, p(f), p(f), p(f), p(f),
                                                          kw.get("prior", p(d)), kw.get("rnd", 0), T, P, R, A, G, p(out), p(out), p(out), p(out),
                                                          p(out), p(i), p(d), Hh._stream())
    for T, P in ((3, 4), (5, 2), (3, 0), (0, 1), (6, 1), (4, 3)):
        assert call(T, P, 2, 4, 4) == -2, (T, P)
    assert call(3, 1, 0, 4, 4) == -2 and call(3, 1, 2, 0, 4) == -2 and call(3, 1, 2, 4, 0) == -2 and call(3, 1, 2, 4, 4, rnd=-1) == -2
    assert call(3, 1, 2, 4, 4, presence=None) == -1 and call(3, 1, 2, 4, 4, prior=None) == -1
    src = lambda C, R, **kw: L.air_propose_source(kw.get("a", p(i)), p(i), C, R, kw.get("o", p(i)), Hh._stream())
    assert src(0, 2) == -2 and src(7, 2) == -2 and src(3, 0) == -2 and src(3, 2, a=None) == -1 and src(3, 2, o=None) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL_F).all() and (i == SENTINEL_I).all() and (d == SENTINEL_F).all()


# ---- 3. a planted scene through the entries ---------------------------------------------------------------------------------------------
CENTRES = [(-0.5, -0.5), (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5)]


def blob_rows(idx, B, crop, scale=0.3, junk=()):
    """rows of ones-glimpses at the given centres (an index into CENTRES, or "junk": a small blob in the middle, where no object is)"""
    h, w = crop
    where = np.zeros((len(idx), B, 4), np.float32)
    where[..., 0::2] = scale
    for j, i in enumerate(idx):
        if i == "junk":
            where[j, :, 0::2], where[j, :, 1], where[j, :, 3] = 0.15, 0.0, 0.0
        else:
            where[j, :, 1], where[j, :, 3] = CENTRES[i]
    return np.ones((len(idx), B, h, w), np.float32), where


def through_the_entries(start_idx, prop_idx, obs_idx, n, prior, T, P):
    """pool -> air_prune_score -> air_prune_select (T := C) -> air_propose_source on a planted scene; returns (device results, float64
    reference)"""
    from attend_infer_repeat_amd import hip as Hh, propose, prune
    (H, W), (h, w), B, A = (16, 16), (4, 4), len(n), 6
    C = T + P
    rng = np.random.default_rng(0)
    g_s, w_s = blob_rows(start_idx, B, (h, w))
    g_p, w_p = blob_rows(prop_idx + [prop_idx[-1]] * (T - len(prop_idx)), B, (h, w))       # the engine leaves T proposal rows; P are used
    g_o, w_o = blob_rows(obs_idx, B, (h, w))
    layers_o = f64_layers(dict(glimpse=g_o, where=w_o, img=(H, W), T=len(obs_idx)))
    obs = (MULT * layers_o.sum(0)).astype(np.float32)
    what_s, what_p = (rng.normal(size=(T, B, A)) * 0.3).astype(np.float32), (rng.normal(size=(T, B, A)) * 0.3).astype(np.float32)
    sc_s, sc_p = np.full((T, B), 0.5, np.float32), np.full((T, B), 0.25, np.float32)
    L, p = Hh.lib(), Hh._p
    d = dict(what=dev_t(what_s), where=dev_t(w_s), glimpse=dev_t(g_s), score=dev_t(sc_s), presence=dev_t(chain(n, T)), pw=dev_t(what_p),
             pwh=dev_t(w_p), pg=dev_t(g_p), ps=dev_t(sc_p), prior=dev_t(np.asarray(prior, np.float64)))
    pool = dict(what=torch.zeros(C, B, A).cuda(), where=torch.zeros(C, B, 4).cuda(), glimpse=torch.zeros(C, B, h * w).cuda(),
                score=torch.zeros(C, B).cuda(), presence=torch.zeros(C, B).cuda(), source=torch.zeros(C, B, dtype=torch.int32).cuda(),
                prior=torch.zeros(C + 1, dtype=torch.float64).cuda())
    st = L.air_propose_pool(p(d["what"]), p(d["where"]), p(d["glimpse"]), p(d["score"]), p(d["presence"]), None, None, p(d["pw"]), p(d["pwh"]),
                            p(d["pg"]), p(d["ps"]), p(d["prior"]), 0, T, P, B, A, h * w, p(pool["what"]), p(pool["where"]), p(pool["glimpse"]),
                            p(pool["score"]), p(pool["presence"]), p(pool["source"]), p(pool["prior"]), Hh._stream())
    torch.cuda.synchronize()
    assert st == 0
    host = {k: v.cpu().numpy() for k, v in pool.items()}
    case = dict(glimpse=host["glimpse"].reshape(C, B, h, w), where=host["where"], presence=host["presence"], obs=obs, img=(H, W), crop=(h, w),
                T=C, B=B)
    rec_ref = prune.reference_score(case["glimpse"], case["where"], case["presence"], obs, MULT, STD, 1, layers=f64_layers(case))
    sel = dict(what=host["what"], where=host["where"], glimpse=host["glimpse"], score=host["score"], presence=host["presence"],
               where_loc=host["where"])
    ref = prune.reference_select(**sel, priors=PRIORS, prior=host["prior"], normalize_prior=1, all_candidates=1, rec_sub=rec_ref)
    rec_sub, st = run_score(case, 1)
    assert st == 0
    got, st = run_select(dict(sel, rec_sub=rec_sub.cpu().numpy()), PRIORS, host["prior"], 1, 1)
    assert st == 0
    src = torch.zeros(C, B, dtype=torch.int32).cuda()
    st = L.air_propose_source(p(pool["source"]), p(got["kept_step"]), C, B, p(src), Hh._stream())
    torch.cuda.synchronize()
    assert st == 0
    got["source_out"] = src
    return got, ref


def test_planted_scene_keeps_the_real_rows_and_the_real_proposal(gpu_device):
    """obs = three blobs; the start rows hold two of them and a spurious row between them; the proposals hold the missing blob and a
    junk row.  The winner keeps the two real start rows and the real proposal."""
    T, P = 3, 2
    n = np.array([3, 1, 0, 2])
    got, ref = through_the_entries([0, 3, 1], [2, "junk"], [0, 1, 2], n, [0.1, 0.2, 0.3, 0.4], T, P)
    finite = np.isfinite(ref["J_sub"])
    order = np.sort(np.where(finite, ref["J_sub"], -np.inf), axis=1)[:, ::-1]
    bar = 2 * OUT_TOL * np.abs(ref["J_sub"][finite]).max()
    expect = 0b01101                                               # pool rows 0 and 2 (start steps 0, 2) and row 3 (proposal 0)
    assert ref["best_mask"].tolist() == [expect] * 4 and (order[:, 0] - order[:, 1] > bar).all()      # the float64 winner, by more than the bar
    assert got["best_mask"].cpu().tolist() == [expect] * 4 and got["num_objects_out"].cpu().tolist() == [3] * 4
    kept, src = got["kept_step"].cpu().numpy(), got["source_out"].cpu().numpy()
    assert (kept == np.array([0, 2, 3, 1, 4])[:, None]).all() and np.array_equal(src, kept)      # round 0: provenance = pool position
    ev = got["evidence"].cpu().numpy()
    assert ev[1, 3] < 0 and ev[3, 3] > 0 and ev[4, 3] < 0         # image 3 (n = 2): the spurious row and the junk are unwanted, the proposal wanted
    assert ev[1, 0] < 0 and np.isneginf(ev[3, 0])                 # image 0 (n = 3): a fourth object is beyond the padded prior
    J = got["J_sub"].cpu().numpy()
    pop = np.array([bin(m).count("1") for m in range(32)])
    assert np.isneginf(J[:, pop > T]).all() and np.isfinite(J[:, pop <= T]).all()


def test_planted_scene_with_four_objects_returns_exactly_T(gpu_device):
    """four real objects, T = 3: the start holds three, the proposal is the fourth -- the padded prior keeps the count at three"""
    T, P = 3, 2
    n = np.array([3, 2, 0])
    got, ref = through_the_entries([0, 1, 2], [3, "junk"], [0, 1, 2, 3], n, [0.1, 0.2, 0.3, 0.4], T, P)
    assert ref["num_objects"].tolist() == [3, 3, 3] and got["num_objects_out"].cpu().tolist() == [3, 3, 3]
    best = got["best_mask"].cpu().numpy()
    assert ((best >> 4) == 0).all()                                # never the junk
    own = _select_on(got, n, T + P)
    assert np.array_equal(best, own)
    assert (got["objective"].cpu().numpy() >= got["objective_start"].cpu().numpy()).all()


def _select_on(got, n, C):
    from attend_infer_repeat_amd import prune
    return prune.select_masks(got["J_sub"].cpu().numpy(), np.asarray(n), C, True)


# ---- 4. ParseProposer behind the providers ------------------------------------------------------------------------------------------------
def make_proposer(name, proposals=1, rounds=1, particles=None, refine=None, capture=False, **cfg_kw):
    from attend_infer_repeat_amd.propose import ParseProposer
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
    pp = ParseProposer(ps, proposals, rounds)
    pp.load_parameters(params)
    pp.set_global_step(20000)
    if capture:
        base.capture()
        if ps is not base:
            ps.capture()
        pp.capture()
    return pp, ocfg, B, params, obs


def check_rounds(pp, ocfg, base, obs, out, label):
    """every round of one call: the pool against the reference pool, the joints against float64 fed with the device's own pool rows, the
    decision on the device's own joints, the provenance, and the round invariants.  `base`: the provider's result (host)."""
    from attend_infer_repeat_amd import propose, prune
    T, B, P, C, Rn = pp.T, pp.R, pp.proposals, pp.C, pp.rounds
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    mult, std = float(ocfg.output_multiplier), float(ocfg.output_std)
    priors = (*ocfg.what_prior, *ocfg.where_scale_prior, *ocfg.where_shift_prior)
    table = pp.engine.prior_dev.cpu().numpy()
    np_ = lambda t: t.detach().cpu().numpy()
    obs_np = obs.reshape(B, H, W).numpy()
    cur = dict(what=np_(base["what"]), where=np_(base["where"]), glimpse=np_(base["glimpse"]).reshape(T, B, -1), score=np_(base["score"]))
    n = prune.leading_ones(np_(base["presence"]))
    assert np.array_equal(np_(out["num_objects_start"]), n)
    src_in, kept_m0 = None, np.ones(B, bool)
    obj = np_(pp.objective_rounds)
    pop = np.array([bin(m).count("1") for m in range(1 << C)])
    for r in range(Rn):
        pool = {k: np_(getattr(pp, "pool_" + k)[r]) for k in ("what", "where", "glimpse", "score", "presence", "source")}
        ref_pool = propose.reference_pool(cur["what"], cur["where"], cur["glimpse"], cur["score"], n, pool["what"][T:], pool["where"][T:],
                                          pool["glimpse"][T:], pool["score"][T:], table, P, round=r, source_in=src_in)
        for k in pool:
            assert np.array_equal(pool[k].view(np.int32), np.ascontiguousarray(ref_pool[k]).view(np.int32)), (r, k)
        assert np.array_equal(np_(pp.pool_prior), ref_pool["prior"])
        case = dict(glimpse=pool["glimpse"].reshape(C, B, h, w), where=pool["where"], img=(H, W), T=C)
        rec = prune.reference_score(case["glimpse"], case["where"], pool["presence"], obs_np, mult, std, 1, layers=f64_layers(case))
        sel_in = (pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, priors, ref_pool["prior"], 1, 1, rec)
        ref = prune.reference_select(*sel_in)
        J = np_(pp.J_sub[r])
        finite = np.isfinite(ref["J_sub"])
        assert np.array_equal(np.isneginf(J), np.isneginf(ref["J_sub"])) and np.array_equal(np.isneginf(J), np.broadcast_to(pop > T, J.shape))
        assert not np.isnan(J).any()
        check_tensor("propose", "%s_round%d" % (label, r), "out", "J_sub", torch.from_numpy(J[finite]), torch.from_numpy(ref["J_sub"][finite]),
                     OUT_TOL, OUT_L2)
        own = prune.reference_select(*sel_in, J_sub=J)             # the rule on the DEVICE's joints: exact, no image left out
        assert np.array_equal(np_(pp.best_mask[r]), own["best_mask"])
        assert np.array_equal(np_(pp.kept_pool[r]), own["kept_step"])
        assert np.array_equal(np_(pp.num_objects_round[r]), own["num_objects"]) and (own["num_objects"] <= T).all()
        assert np.array_equal(obj[r + 1], own["objective"]) and np.array_equal(np_(pp.objective_start_rounds[r]), own["objective_start"])
        assert np.array_equal(np_(pp.evidence[r]), own["evidence"], equal_nan=True)
        for k in ("what", "where", "glimpse", "score"):
            assert np.array_equal(np_(getattr(pp, "out_" + k)[r]).view(np.int32), np.ascontiguousarray(own[k]).view(np.int32)), (r, k)
        src_out = propose.reference_source(pool["source"], own["kept_step"])
        assert np.array_equal(np_(pp.source_out[r]), src_out)
        e = np_(pp.residual_energy[r])
        assert np.isfinite(e).all() and (e >= 0).all()
        kept_m0 &= own["best_mask"] == (1 << n) - 1
        print("propose %s round %d: n %s -> best masks %s, objective gain max %.3g" % (
            label, r, n.tolist(), [bin(m) for m in own["best_mask"]], float((own["objective"] - own["objective_start"]).max())))
        cur = {k: own[k][:T] for k in ("what", "where", "glimpse", "score")}
        n, src_in = own["num_objects"], src_out
    # the invariants
    assert (obj[1:] >= obj[:-1]).all()                             # never worse, round after round
    for r in range(1, Rn):
        assert np.array_equal(np_(pp.objective_start_rounds[r]), obj[r])      # bit for bit: the compaction keeps step order
    assert np.array_equal(np_(out["objective"]), obj[-1]) and np.array_equal(np_(out["objective_start"]), obj[0])
    assert np.array_equal(np_(out["kept_step"]), src_in[:T]) and np.array_equal(np_(out["num_objects"]), n)
    assert np.array_equal(np_(out["objects_proposed_kept"]), ((src_in[:T] >= T) & (np.arange(T)[:, None] < n[None, :])).sum(0))
    assert same_bits(out["proposal_what"], pp.pool_what[:, T:].cpu()) and tuple(out["proposal_glimpse"].shape) == (Rn, P, B, h, w)
    assert tuple(out["residual"].shape) == (B, H, W) and tuple(out["residual_energy"].shape) == (Rn, B)
    return cur, n, kept_m0


def check_residual_of_the_last_round(pp, ocfg, base_dev, out):
    """the residual the proposal engine saw in the last round: bit-equal to clamp(obs - air_parse_render's reconstruction) of that
    round's current rows; its energy within the bars of float64 on those bits"""
    T, B, Rn = pp.T, pp.R, pp.rounds
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    if Rn == 1:
        g, wh, pres = base_dev["glimpse"], base_dev["where"], base_dev["presence"]
    else:
        g, wh = pp.out_glimpse[Rn - 2, :T].view(T, B, h, w), pp.out_where[Rn - 2, :T]
        pres = (torch.arange(T, device=g.device)[:, None] < pp.num_objects_round[Rn - 2][None, :]).float()
    obs = pp._start["obs"].view(B, H, W)
    r = run_render(g.contiguous(), wh.contiguous(), pres.contiguous(), obs, float(ocfg.output_multiplier), float(ocfg.output_std), (H, W),
                   (h, w), layers=False)
    diff = obs - r["reconstruction"]
    want = torch.where(diff > 0, torch.clamp(diff, max=pp.clamp_hi), torch.zeros_like(diff))
    assert torch.equal(out["residual"], want)
    e64 = (want.double() ** 2).reshape(B, -1).sum(1).cpu()
    check_tensor("propose", "residual_energy", "out", "residual_energy", out["residual_energy"][-1].cpu(), e64, OUT_TOL, OUT_L2)


def check_readout(pp, ocfg, out_dev, out, base, n, kept_m0):
    """the read-out against air_parse_objects / air_parse_render on the first T compacted rows, bit for bit; images that kept their
    start mask in every round return the provider's parse bit for bit"""
    T, B = pp.T, pp.R
    (H, W), (h, w) = ocfg.img_size, ocfg.crop_size
    hand = run_objects(out_dev["presence_prob"], out_dev["num_objects"], out_dev["where"].contiguous(), out_dev["what"].contiguous(), H, W)
    for k in ("num_objects", "count_prob", "presence", "boxes", "offsets"):
        assert same_bits(out_dev[k], hand[k]), k
    rows = int(out["offsets"][-1])
    for k in ("obj_image", "obj_box", "obj_where", "obj_what"):
        assert same_bits(out_dev[k][:rows], hand[k][:rows]), k
    kept_rows = np.arange(T)[:, None] < n[None, :]
    score_src = pp.out_score[-1, :T].cpu().numpy()
    assert np.array_equal(out["score"].numpy(), np.where(kept_rows, score_src, hand["score"].cpu().numpy()), equal_nan=True)
    for b in range(B):
        lo, hi = int(out["offsets"][b]), int(out["offsets"][b + 1])
        assert hi - lo == n[b] and out["obj_step"][lo:hi].tolist() == out["kept_step"][:hi - lo, b].tolist()
        assert np.array_equal(out["obj_score"][lo:hi].numpy(), score_src[:hi - lo, b])
    rend = run_render(out_dev["glimpse"].contiguous(), out_dev["where"].contiguous(), out_dev["presence"], pp._start["obs"].view(B, H, W),
                      float(ocfg.output_multiplier), float(ocfg.output_std), (H, W), (h, w), layers=False)
    for k in ("reconstruction", "owner", "area", "rec"):
        assert same_bits(out_dev[k], rend[k]), k
    for b in np.nonzero(kept_m0)[0]:
        for k in base:
            if k in ("offsets", "layers") or k not in out:
                continue
            v, u = out[k], base[k]
            if k in ("objective", "objective_start"):              # behind a refiner these are the refiner's under another name
                continue
            if k.startswith("obj_"):
                assert same_bits(v[int(out["offsets"][b]):int(out["offsets"][b + 1])], u[int(base["offsets"][b]):int(base["offsets"][b + 1])]), k
            elif v.dim() > 1 and v.shape[0] == T and v.shape[1] == B:
                assert same_bits(v[:, b], u[:, b]), k
            elif v.shape[0] == B:
                assert same_bits(v[b], u[b]), k
    return int(kept_m0.sum())


PRUNER_KEYS = {"objective", "objective_start", "objective_subsets", "best_mask", "kept_step", "evidence", "num_objects_start"}
NEW_KEYS = PRUNER_KEYS | {"objective_rounds", "residual", "residual_energy", "proposal_what", "proposal_where", "proposal_glimpse",
                          "proposal_score", "objects_proposed_kept"}


@pytest.mark.parametrize("name,proposals,rounds", [("tiny", 1, 1), ("tiny", 3, 2), ("mnist_b8", 1, 2), ("mnist_b8", 3, 1), ("rect_t5", 1, 2)])
def test_proposer_behind_a_scene_parser(gpu_device, name, proposals, rounds):
    pp, ocfg, B, params, obs = make_proposer(name, proposals, rounds)
    counts = mixed_counts(ocfg, B)
    base_dev = pp.parser.parse(obs.cuda(), counts)
    pp.synchronize()
    base = cpu(base_dev)
    out_dev = pp.parse(obs.cuda(), counts)
    pp.synchronize()
    torch.cuda.synchronize()
    out = cpu(out_dev)
    assert set(out) == set(base) | NEW_KEYS
    label = "%s_P%d_R%d" % (name, proposals, rounds)
    cur, n, kept_m0 = check_rounds(pp, ocfg, base, obs, out, label)
    check_residual_of_the_last_round(pp, ocfg, base_dev, out_dev)
    same = check_readout(pp, ocfg, out_dev, out, base, n, kept_m0)
    print("propose %s: %d of %d images kept their start mask throughout" % (label, same, B))
    for k in ("presence_prob", "num_steps_posterior"):
        assert same_bits(out[k], base[k]), k
    # the proposals are the proposal engine's first P steps of its last pass (the pool archives every round's)
    ie = pp.proposal.engine
    assert same_bits(out_dev["proposal_what"][-1], ie.what[:proposals]) and same_bits(out_dev["proposal_where"][-1], ie.where[:proposals])
    assert same_bits(out_dev["proposal_score"][-1], ie.step_w[:proposals])
    assert same_bits(out_dev["proposal_glimpse"][-1].reshape(proposals, B, -1), ie.gd.out[-1].view(pp.T, B, -1)[:proposals])
    # ... and that pass is the engine's forward plan at the mode on the residual: a plain SceneParser shown the residual agrees
    twin = make_parser(ocfg, B, params)
    t = twin.parse(out_dev["residual"].clone())
    twin.synchronize()
    assert same_bits(t["what"][:proposals], out_dev["proposal_what"][-1]) and same_bits(t["where"][:proposals], out_dev["proposal_where"][-1])
    assert pp.launch_count()["propose_residual"] == rounds and len(pp._plan) == rounds * (6 + len(ie._plan_fwd)) + 4


@pytest.mark.parametrize("name,particles,refine,proposals,rounds", [("mnist_b8", 4, None, 1, 2), ("tiny", None, 2, 2, 1), ("rect_t5", 4, 2, 1, 1)])
def test_proposer_behind_the_other_providers(gpu_device, name, particles, refine, proposals, rounds):
    pp, ocfg, B, params, obs = make_proposer(name, proposals, rounds, particles=particles, refine=refine)
    args = () if particles is not None else (mixed_counts(ocfg, B),)
    kw = {} if particles is None else dict(sample_noise=False)
    if particles is not None:
        pp.parser.parse(obs.cuda())                                # draw noise once; the calls below keep it
    base_dev = pp.parser.parse(obs.cuda(), *args, **kw)
    pp.synchronize()
    base = cpu(base_dev)
    out_dev = pp.parse(obs.cuda(), *args, **kw)
    pp.synchronize()
    torch.cuda.synchronize()
    out = cpu(out_dev)
    assert "layers" not in out and set(base) - {"layers"} <= set(out) and NEW_KEYS <= set(out)
    for k in ("presence_prob", "num_steps_posterior"):
        assert same_bits(out[k], base[k]), k
    if refine is not None:
        assert same_bits(out["refine_objective"], base["objective"]) and same_bits(out["refine_objective_start"], base["objective_start"])
    label = "%s_K%s_refine%s_P%d_R%d" % (name, particles, refine, proposals, rounds)
    cur, n, kept_m0 = check_rounds(pp, ocfg, base, obs, out, label)
    check_residual_of_the_last_round(pp, ocfg, base_dev, out_dev)
    check_readout(pp, ocfg, out_dev, out, base, n, kept_m0)


# ---- 5. a planted scene through the module's segments; graph replay -----------------------------------------------------------------------
PLANTED_N = [3, 1, 2, 3, 0, 2, 1, 3]
PLANTED_SAME = (3, 7)                                              # images whose obs IS the start parse (n = 3): m0 stays


def run_segment(pp, seg):
    pp.engine._replay_or_run(None, seg)


def test_planted_scene_through_the_module(gpu_device):
    """The provider's bound start buffers are overwritten with a planted scene (three blobs; the start rows hold two of them and a
    spurious row between them) and the state a provider would have returned for it; the segments then run eagerly one at a time, and
    behind `forward` the proposal engine's first P rows are overwritten with the missing blob and a junk row."""
    from attend_infer_repeat_amd import prune
    P = 2
    pp, ocfg, B, params, obs0 = make_proposer("mnist_b8", P, 1)
    T, C, (H, W), (h, w), A = pp.T, pp.C, ocfg.img_size, ocfg.crop_size, ocfg.n_appearance
    assert (T, B, C) == (3, 8, 5)
    mult, std = float(ocfg.output_multiplier), float(ocfg.output_std)
    par, st, eng, ie = pp.parser, pp._start, pp.engine, pp.proposal.engine
    first = pp.parse(obs0.cuda(), mixed_counts(ocfg, B))           # binds, checks the buffers, fills presence_prob and the count table
    pp.synchronize(); torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    g_s, w_s = blob_rows([0, 3, 1], B, (h, w))
    g_p, w_p = blob_rows([2, "junk"], B, (h, w))
    layers = f64_layers(dict(glimpse=np.concatenate([g_s, g_p[:1]], 0), where=np.concatenate([w_s, w_p[:1]], 0), img=(H, W), T=4))
    canvas = layers[0] + layers[2] + layers[3]                     # blobs 0, 1 and 2
    for b in PLANTED_SAME:
        canvas[b] = layers[0][b] + layers[1][b] + layers[2][b]     # ... or exactly the start rows
    obs = (mult * canvas).astype(np.float32)
    what_s, what_p = (rng.normal(size=(T, B, A)) * 0.3).astype(np.float32), (rng.normal(size=(P, B, A)) * 0.3).astype(np.float32)
    n = torch.tensor(PLANTED_N, dtype=torch.int32).cuda()
    st["what"].copy_(dev_t(what_s)); st["where"].copy_(dev_t(w_s)); st["glimpse"].copy_(dev_t(g_s).reshape(st["glimpse"].shape))
    st["obs"].copy_(dev_t(obs).reshape(st["obs"].shape))
    prov = run_objects(st["presence_prob"], n, st["where"], st["what"], H, W)
    par.presence.copy_(prov["presence"]); par.score.copy_(prov["score"]); par.num_objects.copy_(prov["num_objects"])
    torch.cuda.synchronize()
    seg = pp.segments[0]
    run_segment(pp, seg["residual"]); run_segment(pp, seg["forward"])
    pp.synchronize()
    # the residual of the planted scene: the missing blob where the start has objects 0 and 1, nothing where obs is the start parse
    res = pp.residual.cpu().numpy()
    assert np.abs(res[0] - mult * layers[3][0]).max() <= OUT_TOL * mult + 1e-6 and np.abs(res[list(PLANTED_SAME)]).max() <= 1e-6
    ie.what[:P].copy_(dev_t(what_p)); ie.where[:P].copy_(dev_t(w_p))
    ie.gd.out[-1].view(T, B, h * w)[:P].copy_(dev_t(g_p).reshape(P, B, h * w)); ie.step_w[:P].fill_(0.25)
    torch.cuda.synchronize()
    for name in ("pool", "score", "select", "source"):
        run_segment(pp, seg[name])
    run_segment(pp, pp.readout)
    pp.synchronize(); torch.cuda.synchronize()
    out_dev = pp._result({k: first[k] for k in first if k not in NEW_KEYS})
    out = cpu(out_dev)
    # the float64 winner on the device's pool rows, by more than the bar
    pool = {k: getattr(pp, "pool_" + k)[0].cpu().numpy() for k in ("what", "where", "glimpse", "score", "presence")}
    case = dict(glimpse=pool["glimpse"].reshape(C, B, h, w), where=pool["where"], img=(H, W), T=C)
    rec = prune.reference_score(case["glimpse"], case["where"], pool["presence"], obs, mult, std, 1, layers=f64_layers(case))
    priors = (*ocfg.what_prior, *ocfg.where_scale_prior, *ocfg.where_shift_prior)
    ref = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, priors,
                                 pp.pool_prior.cpu().numpy(), 1, 1, rec)
    expect = [0b00111 if b in PLANTED_SAME else 0b01101 for b in range(B)]
    finite = np.isfinite(ref["J_sub"])
    order = np.sort(np.where(finite, ref["J_sub"], -np.inf), axis=1)[:, ::-1]
    bar = 2 * OUT_TOL * np.abs(ref["J_sub"][finite]).max()
    assert ref["best_mask"].tolist() == expect and (order[:, 0] - order[:, 1] > bar).all()
    assert out["best_mask"].tolist() == expect and out["num_objects"].tolist() == [3] * B
    truth = [b for b in range(B) if b not in PLANTED_SAME]
    kept = out["kept_step"].numpy()
    assert (kept[:, truth] == np.array([0, 2, T + 0])[:, None]).all() and (kept[:, list(PLANTED_SAME)] == np.array([0, 1, 2])[:, None]).all()
    assert out["objects_proposed_kept"].tolist() == [0 if b in PLANTED_SAME else 1 for b in range(B)]
    assert (out["objective"] > out["objective_start"])[truth].all() and (out["objective"] == out["objective_start"])[list(PLANTED_SAME)].all()
    # reconstruction, owner map and object table describe the three real blobs
    assert np.abs(out["reconstruction"].numpy() - obs).max() <= OUT_TOL * np.abs(obs).max()
    assert (out["area"].numpy() > 0).all()
    px = lambda c: (int(round((c[1] + 1) / 2 * (H - 1))), int(round((c[0] + 1) / 2 * (W - 1))))      # (row, column) of a centre
    for b in truth:
        assert [int(out["owner"][b][px(CENTRES[i])]) for i in (0, 1, 2)] == [0, 1, 2] and int(out["owner"][b][px(CENTRES[3])]) == -1
        lo, hi = int(out["offsets"][b]), int(out["offsets"][b + 1])
        assert hi - lo == 3 and out["obj_step"][lo:hi].tolist() == [0, 2, T + 0] and (out["obj_image"][lo:hi] == b).all()
        assert np.array_equal(out["obj_where"][lo:hi].numpy(), np.stack([w_s[0, b], w_s[2, b], w_p[0, b]]))
        assert np.array_equal(out["obj_what"][lo:hi].numpy(), np.stack([what_s[0, b], what_s[2, b], what_p[0, b]]))
        assert out["obj_score"][lo:hi].tolist()[2] == 0.25
    check_readout(pp, ocfg, out_dev, out, {}, np.array([3] * B), np.zeros(B, bool))


@pytest.mark.parametrize("name,particles,proposals,rounds", [("mnist_b8", None, 1, 2), ("tiny", 4, 3, 1)])
def test_graph_replay_equals_eager(gpu_device, name, particles, proposals, rounds):
    from oracle import air_oracle as O
    eager, ocfg, B, params, _ = make_proposer(name, proposals, rounds, particles=particles)
    graph = make_proposer(name, proposals, rounds, particles=particles, capture=True)[0]
    assert graph._graph is not None and eager._graph is None
    kw = {} if particles is None else dict(sample_noise=False)
    args = (mixed_counts(ocfg, B),) if particles is None else ()
    noise = O.make_noise(ocfg, B * (particles or 1), seed=5)
    for pp in (eager, graph):
        if particles is not None:
            pp.engine.set_noise(noise["eps_where"].cuda(), noise["eps_what"].cuda(), noise["u_pres"].cuda())
    kept = []
    for seed in (11, 12):
        obs = O.synthetic_batch(ocfg, B, seed=seed)[0].cuda()
        a, b = eager.parse(obs, *args, **kw), graph.parse(obs, *args, **kw)
        eager.synchronize(); graph.synchronize(); torch.cuda.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
        kept.append(b["objective_subsets"].clone())
    assert not same_bits(kept[0], kept[1])
    # update_config re-captures: a changed output_multiplier changes the joints, and changing it back restores the bits
    assert graph.update_config(output_multiplier=0.25) and graph._graph is not None
    c = graph.parse(obs, *args, **kw)["objective_subsets"].clone()
    assert not same_bits(c, kept[1])
    assert graph.proposal.engine.cfg.output_multiplier == 0.25
    assert graph.update_config(output_multiplier=float(ocfg.output_multiplier))
    assert same_bits(graph.parse(obs, *args, **kw)["objective_subsets"], kept[1])
    graph.release_graphs(); graph.parser.release_graphs()


def test_set_global_step_moves_the_joints_by_the_change_of_log_pi(gpu_device):
    pp, ocfg, B, params, obs = make_proposer("tiny", 1, 1)
    T, C = pp.T, pp.C
    counts = mixed_counts(ocfg, B)
    tables, joints, props = [], [], []
    for step in (20000, 40000):
        pp.set_global_step(step)
        out = pp.parse(obs.cuda(), counts)
        pp.synchronize(); torch.cuda.synchronize()
        tables.append(pp.engine.prior_dev.cpu().numpy().copy())
        joints.append(out["objective_subsets"].cpu().numpy().copy())
        props.append(out["proposal_what"].clone())
    assert not np.array_equal(tables[0], tables[1])                 # the count prior is annealed: the two steps differ
    assert np.array_equal(pp.proposal.engine.prior_dev.cpu().numpy(), tables[1]) and same_bits(props[0], props[1])
    logpi = [np.log(t / t.sum()) for t in tables]
    pop = np.array([bin(m).count("1") for m in range(1 << C)])
    live = pop <= T
    delta = (logpi[1] - logpi[0])[pop[live]][None, :]
    assert np.abs((joints[1][:, live] - joints[0][:, live]) - delta).max() <= 1e-9 * (1 + np.abs(joints[0][:, live]).max())
    assert np.isneginf(joints[0][:, ~live]).all() and np.isneginf(joints[1][:, ~live]).all()


# ---- 6. scoring, the model and the surface ------------------------------------------------------------------------------------------------
def test_scorer_bound_to_a_proposer_scores_the_proposed_parse(gpu_device):
    from attend_infer_repeat_amd.score import ParseScorer
    from test_score import annotated_batches
    pp, ocfg, B, params, _ = make_proposer("mnist_b8", 1, 1)
    G = 2
    fake = types.SimpleNamespace(engine=pp.engine, T=pp.T, R=pp.R, **{k: torch.zeros_like(getattr(pp, k)) for k in
                                                                     ("owner", "boxes", "num_objects", "score", "presence")})
    sc, sc_hand = ParseScorer(pp, G, max_batches=4), ParseScorer(fake, G, max_batches=4)
    for i, b in enumerate(annotated_batches("mnist_b8", B, 2, seed=3)):
        out = pp.parse(torch.from_numpy(b["obs"]).cuda(), mixed_counts(ocfg, B))
        for k in ("owner", "boxes", "num_objects", "score", "presence"):
            assert out[k].data_ptr() == getattr(pp, k).data_ptr()
            getattr(fake, k).copy_(out[k])
        sc.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
        sc_hand.score(b["instances"], torch.from_numpy(b["boxes"]).cuda(), accumulate=i > 0)
    a, h = sc.summary(), sc_hand.summary()
    assert set(a) == set(h) and a["images"] == 2 * B
    for k in a:
        assert a[k] == h[k] or (math.isnan(a[k]) and math.isnan(h[k])), k


def test_proposing_on_the_model_does_not_disturb_training(gpu_device):
    B, T, A = 8, 3, 50
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    before = _train_state(air._engine)
    plain = {k: v.clone() for k, v in air.parse().items()}
    out = air.parse(propose=1)
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert out is air.parsed and set(out) - set(plain) == NEW_KEYS
    h, w = out["glimpse"].shape[-2:]
    assert {k: tuple(out[k].shape) for k in NEW_KEYS} == {
        "objective": (B,), "objective_start": (B,), "objective_subsets": (B, 16), "best_mask": (B,), "kept_step": (T, B),
        "evidence": (T + 1, B), "num_objects_start": (B,), "objective_rounds": (2, B), "residual": (B, 50, 50), "residual_energy": (1, B),
        "proposal_what": (1, 1, B, A), "proposal_where": (1, 1, B, 4), "proposal_glimpse": (1, 1, B, h, w), "proposal_score": (1, 1, B),
        "objects_proposed_kept": (B,)}
    assert out["objective"].dtype == torch.float64 and out["kept_step"].dtype == torch.int32 and out["objects_proposed_kept"].dtype == torch.int32
    assert torch.equal(out["num_objects_start"], plain["num_objects"])
    for k in ("presence_prob", "num_steps_posterior"):
        assert torch.equal(out[k], plain[k]), k
    assert (out["objective"] >= out["objective_start"]).all() and torch.isfinite(out["reconstruction"]).all()
    assert (out["num_objects"] <= T).all() and torch.equal(out["presence"].sum(0).int(), out["num_objects"])
    assert (out["residual"] >= 0).all() and (out["residual"] <= 1).all()
    # the pool search contains prune="all": never below it, and the two exclude each other
    pruned = air.parse(prune="all")["objective"].clone()
    again_p = air.parse(propose=1)
    assert (again_p["objective"] >= pruned).all()
    with pytest.raises(ValueError, match="prune together with propose"):
        air.parse(prune="all", propose=1)
    with pytest.raises(ValueError, match="prune together with propose"):
        air.parse_scorer(2, prune="present", propose=1)
    for bad in ("one", (1, 2, 3), True):
        with pytest.raises(ValueError, match="propose"):
            air.parse(propose=bad)
    with pytest.raises(ValueError, match="proposals"):
        air.parse(propose=4)                                       # more proposals than the pass has steps
    # cached per (provider, proposals, rounds), LRU-bounded; propose=None is the old path, bit for bit
    assert len(air._parse_proposers) == 1 and air.parse(propose=1) is air.parsed and len(air._parse_proposers) == 1
    two = air.parse(propose=(1, 2))
    assert tuple(two["objective_rounds"].shape) == (3, B) and len(air._parse_proposers) == 2
    assert (two["objective_rounds"][1:] >= two["objective_rounds"][:-1]).all()
    for spec in (2, 3, (2, 2), (3, 2)):
        air.parse(propose=spec)
    assert len(air._parse_proposers) == air.MAX_PARSE_PROPOSERS == 4
    again = air.parse()
    assert set(again) == set(plain) and all(torch.equal(again[k], plain[k]) for k in plain)
    both = air.parse(particles=2, refine=1, propose=1)
    assert NEW_KEYS | {"best_particle", "best_iter", "refine_objective"} <= set(both) and both["objective"].dtype == torch.float64
    assert air._parser_for(2, "joint", 1, None, None, 1).parser is air._parser_for(2, "joint", 1, None)
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # the loggers against a torch recomputation
    from attend_infer_repeat_amd.evaluation import make_parse_logger
    got = make_parse_logger(air, lambda: (x, y), 2, "test", propose=1)(itr=3)
    assert set(got) == {"map_num_step_acc", "count_prob", "num_objects", "objects_added_from_residual", "count_changed", "objective_gain"}
    o = air.parse(x, propose=1)
    gain = o["objective"] - o["objective_start"]
    assert abs(got["objective_gain"] - gain.mean().item()) <= 1e-9 * (1 + abs(gain.mean().item()))
    assert got["count_changed"] == (o["num_objects"] != o["num_objects_start"]).double().mean().item()
    assert got["objects_added_from_residual"] == o["objects_proposed_kept"].double().mean().item()
    assert got["objects_added_from_residual"] == ((o["kept_step"] >= T) & (o["presence"] > 0.5)).double().sum().item() / B
    got_rp = make_parse_logger(air, lambda: (x, y), 1, "test", refine=2, propose=(1, 2))(itr=3)
    assert {"objects_added_from_residual", "count_changed", "objective_gain", "propose_objective_gain", "refine_moved"} <= set(got_rp)
    assert got_rp["propose_objective_gain"] >= 0.0


def test_score_parse_with_proposals_and_the_score_logger(gpu_device):
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.evaluation import make_parse_score_logger
    from attend_infer_repeat_amd.score import ParseScorer
    B = 8
    air, ts, x, y = _mnist_air(B)
    d = procedural_multi_mnist(B, seed=3, n_templates=200, return_annotations=True)
    data = dict(imgs=d["imgs"].astype(np.float32) / 255.0, instances=d["instances"], boxes=d["boxes"])
    air.score_parse(torch.from_numpy(data["imgs"]).cuda(), data["instances"], data["boxes"], accumulate=False, propose=1)
    sc = air.parse_scorer(2, propose=1)
    assert sc.parser is air._parser_for(None, "joint", None, None, None, 1) and sc.parser.proposals == 1
    s = sc.summary()
    assert s["images"] == B
    pp = sc.parser
    fake = types.SimpleNamespace(engine=pp.engine, T=pp.T, R=pp.R, **{k: getattr(pp, k).clone() for k in
                                                                     ("owner", "boxes", "num_objects", "score", "presence")})
    hand = ParseScorer(fake, 2)
    hand.score(data["instances"], data["boxes"], accumulate=False)
    h = hand.summary()
    for k in s:
        assert s[k] == h[k] or (math.isnan(s[k]) and math.isnan(h[k])), k
    got = make_parse_score_logger(air, data, 1, "test", propose=(1, 2))(itr=1)
    assert {"objects_added_from_residual", "count_changed", "objective_gain", "count_acc", "map", "fg_ari"} <= set(got)


def test_training_script_parse_propose_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--parse-eval",
                            "--parse-propose", "1,2"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse+propose([1, 2]) ") == 2
    for l in rec:
        assert l["propose"] == [1, 2] and 0.0 <= l["count_changed"] <= 1.0 and l["objective_gain"] >= 0.0
        assert l["objects_added_from_residual"] >= 0.0
    for bad in (["--parse-propose", "0"], ["--parse-propose", "x"], ["--parse-propose", "1,2,3"], ["--parse-propose", "1", "--parse-prune", "all"]):
        with pytest.raises(SystemExit):
            multi_mnist.main(bad)
