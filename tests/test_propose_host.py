"""Host-side tests of residual proposals (attend_infer_repeat_amd/propose.py): the argument checks, `reference_residual` against a
direct float64 loop, `reference_pool` (layout, provenance, the padded prior), the padded prior keeping the selected count <= T even
when a larger subset reconstructs best, round chaining in numpy, and the new entries in the header and the binding.  No GPU."""
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from attend_infer_repeat_amd import propose, prune
from attend_infer_repeat_amd.engine_config import EngineConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "air_hip.h")
PRIORS = (0.0, 1.0, 0.3, 0.5, 0.0, 1.0)


# ---- 1. check_arguments ---------------------------------------------------------------------------------------------------------
def test_check_arguments_accepts_the_scripts_configuration():
    cfg = EngineConfig(max_steps=3, explore_eps=1e-3, steps_pred_hidden=(128, 64), transform_var_bias=.5, step_bias=.75,
                       output_multiplier=.5)
    propose.check_arguments(cfg)
    propose.check_arguments(cfg, 3, 2)                             # C = 6
    propose.check_arguments(dataclasses.replace(cfg, max_steps=5), 1, 4)
    propose.check_arguments(dataclasses.replace(cfg, mfma_dtype="bf16"), 2)


@pytest.mark.parametrize("change,proposals,rounds,match", [
    (dict(max_steps=3), 4, 1, "proposals"), (dict(max_steps=3), 0, 1, "proposals"), (dict(max_steps=3), -1, 1, "proposals"),
    (dict(max_steps=5), 2, 1, "max_steps \\+ proposals"), (dict(max_steps=4), 3, 1, "max_steps \\+ proposals"),
    (dict(max_steps=6), 1, 1, "max_steps \\+ proposals"), (dict(max_steps=3), 1, 0, "rounds"),
    (dict(max_steps=7), 1, 1, "64 subsets"), (dict(discrete_steps=False), 1, 1, "discrete_steps"),
    (dict(what_prior=None), 1, 1, "what_prior"), (dict(where_scale_prior=None), 1, 1, "where_scale_prior"),
    (dict(where_shift_prior=None), 1, 1, "where_shift_prior"), (dict(where_shift_prior=(None, 1.0)), 1, 1, "loc")])
def test_check_arguments_refuses(change, proposals, rounds, match):
    with pytest.raises(ValueError, match=match):
        propose.check_arguments(dataclasses.replace(EngineConfig(max_steps=3), **change), proposals, rounds)


# ---- 2. reference_residual --------------------------------------------------------------------------------------------------------
def direct_layer(g, wh, H, W):
    """the inverse spatial-transformer write of one glimpse, pixel by pixel (the rule include/air_hip.h states for air_parse_render)"""
    h, w = g.shape
    sx, tx, sy, ty = wh
    out = np.zeros((H, W))
    tap = lambda i, j: g[i, j] if 0 <= i < h and 0 <= j < w else 0.0
    for I in range(H):
        for J in range(W):
            X = -1.0 + 2.0 * J / (W - 1) if W > 1 else -1.0
            Y = -1.0 + 2.0 * I / (H - 1) if H > 1 else -1.0
            cx = ((1.0 / sx) * X + (-tx / sx) + 1.0) * ((w - 1) / 2.0)
            cy = ((1.0 / sy) * Y + (-ty / sy) + 1.0) * ((h - 1) / 2.0)
            if not (-1.0 < cx < w and -1.0 < cy < h):
                continue
            fx, fy = math.floor(cx), math.floor(cy)
            dx, dy = (fx + 1.0) - cx, (fy + 1.0) - cy
            out[I, J] = dx * dy * tap(fy, fx) + (1 - dx) * (1 - dy) * tap(fy + 1, fx + 1) + dx * (1 - dy) * tap(fy + 1, fx) \
                + (1 - dx) * dy * tap(fy, fx + 1)
    return out


def test_reference_residual_against_a_direct_loop():
    (H, W), (h, w), T, B = (5, 7), (3, 2), 3, 4
    rng = np.random.default_rng(0)
    glimpse = rng.normal(size=(T, B, h, w))
    where = np.empty((T, B, 4))
    where[..., 0::2] = rng.uniform(0.4, 1.1, (T, B, 2))
    where[..., 1::2] = rng.normal(size=(T, B, 2)) * 0.4
    where[2, 0, 3] = 6.0                                           # wholly outside
    n = np.array([3, 0, 2, 1])
    obs = rng.uniform(0, 2.5, (B, H, W))
    glimpse[0, 3, 1, 1] = np.nan                                   # a NaN glimpse value: the pixels it reaches give 0
    mult, hi = 0.5, 1.0
    res, energy = propose.reference_residual(glimpse, where, n, obs, mult, hi)
    want = np.zeros((B, H, W))
    for b in range(B):
        canvas = np.zeros((H, W))
        for t in range(n[b]):
            canvas = canvas + direct_layer(glimpse[t, b], where[t, b], H, W)
        d = obs[b] - mult * canvas
        for I in range(H):
            for J in range(W):
                v = d[I, J]
                want[b, I, J] = min(v, hi) if v > 0 else 0.0
    assert np.allclose(res, want, rtol=1e-12, atol=1e-12)
    assert np.allclose(energy, (want ** 2).reshape(B, -1).sum(1), rtol=1e-12)
    assert np.array_equal(res[1], np.minimum(obs[1], hi))          # n = 0: the clamped image itself
    assert (res == hi).any() and (res == 0).any() and (res >= 0).all() and (res <= hi).all()
    nan_px = np.isnan(direct_layer(glimpse[0, 3], where[0, 3], H, W))
    assert nan_px.any() and (res[3][nan_px] == 0).all()


# ---- 3. reference_pool --------------------------------------------------------------------------------------------------------------
def pool_inputs(T, B, A, G, seed):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)
    cur = dict(what=r(T, B, A), where=r(T, B, 4), glimpse=r(T, B, G), score=rng.uniform(size=(T, B)).astype(np.float32))
    prop = dict(prop_what=r(T, B, A), prop_where=r(T, B, 4), prop_glimpse=r(T, B, G), prop_score=rng.uniform(size=(T, B)).astype(np.float32))
    return cur, prop


def test_reference_pool_layout_sources_and_padded_prior():
    T, B, A, G, P = 3, 5, 7, 6, 2
    cur, prop = pool_inputs(T, B, A, G, 1)
    n = np.array([3, 0, 1, 2, 9])                                  # (9 is clipped to T)
    prior = np.array([0.1, 0.2, 0.3, 0.4])
    pool = propose.reference_pool(**cur, n=n, **prop, prior=prior, proposals=P)
    for k in ("what", "where", "glimpse", "score"):
        assert pool[k].shape[0] == T + P and pool[k].dtype == np.float32
        assert np.array_equal(pool[k][:T], cur[k]) and np.array_equal(pool[k][T:], prop["prop_" + k][:P])
    assert pool["presence"].T.tolist() == [[1, 1, 1, 0, 0], [0] * 5, [1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 1, 0, 0]]
    assert pool["source"].dtype == np.int32 and (pool["source"] == np.arange(T + P)[:, None]).all()
    assert pool["prior"].tolist() == [0.1, 0.2, 0.3, 0.4, 0.0, 0.0] and pool["prior"].dtype == np.float64
    # round 2 on rows that came from start step 2, proposal 0 of round 0 and start step 0
    src_in = np.array([[2] * B, [T + 0] * B, [0] * B, [99] * B, [99] * B], np.int32)
    pool2 = propose.reference_pool(**cur, n=n, **prop, prior=prior, proposals=P, round=2, source_in=src_in)
    assert pool2["source"][:, 0].tolist() == [2, 3, 0, T + 2 * P, T + 2 * P + 1]
    kept = np.stack([np.random.default_rng(b).permutation(T + P) for b in range(B)], 1)
    so = propose.reference_source(pool2["source"], kept)
    assert all(so[j, b] == pool2["source"][kept[j, b], b] for j in range(T + P) for b in range(B)) and so.dtype == np.int32


# ---- 4. the padded prior keeps the count <= T -----------------------------------------------------------------------------------------
def test_padded_prior_never_selects_more_than_T_rows():
    T, P, B, A, G = 3, 3, 6, 4, 4
    C = T + P
    cur, prop = pool_inputs(T, B, A, G, 2)
    for d in (cur, prop):
        for k in d:
            d[k] = d[k] * 0.1                                      # small latent terms: the reconstruction term decides
    rng = np.random.default_rng(3)
    n = np.array([3, 0, 1, 2, 3, 0])
    prior = np.array([0.1, 0.2, 0.3, 0.4])
    pool = propose.reference_pool(**cur, n=n, **prop, prior=prior, proposals=P)
    pop = np.array([bin(m).count("1") for m in range(1 << C)])
    rec = rng.uniform(500, 1000, (B, 1 << C))
    rec[:, pop > T] = rng.uniform(0, 1, (B, int((pop > T).sum())))      # every subset above T reconstructs far better
    rec[:, (1 << C) - 1] = 0.0
    for normalize in (0, 1):
        sel = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, PRIORS,
                                     pool["prior"], normalize, True, rec)
        assert (sel["num_objects"] <= T).all() and (sel["num_objects"] == pop[sel["best_mask"]]).all()
        assert np.isneginf(sel["J_sub"][:, pop > T]).all() and np.isfinite(sel["J_sub"][:, pop <= T]).all()
        assert (sel["objective"] >= sel["objective_start"]).all()
        assert (sel["best_mask"] != (1 << n) - 1).any()                # the search is not trivial
        # the kept rows are the first num_objects rows of the compaction: all inside the first T
        for b in range(B):
            assert sorted(sel["kept_step"][:sel["num_objects"][b], b]) == [t for t in range(C) if (sel["best_mask"][b] >> t) & 1]
    # without the padding the larger subsets win: the padding is what holds the count
    flat = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, PRIORS,
                                  np.full(C + 1, 0.1), 1, True, rec)
    assert (flat["num_objects"] > T).all()


# ---- 5. round chaining ----------------------------------------------------------------------------------------------------------------
def test_round_chaining_in_numpy_reproduces_the_objective():
    """two rounds through reference_residual / reference_pool / prune.reference_score / prune.reference_select with fixed `proposal`
    rows: objective_start of round 1 is objective of round 0 bit for bit, and the objective does not decrease"""
    (H, W), (h, w), T, P, B, A = (12, 12), (3, 3), 2, 1, 3, 4
    mult, std = 1.0, 0.3
    rng = np.random.default_rng(4)
    centres = [(-0.5, -0.5), (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5)]

    def rows(idx):
        where = np.zeros((len(idx), B, 4))
        where[..., 0::2] = 0.3
        for j, i in enumerate(idx):
            where[j, :, 1], where[j, :, 3] = centres[i]
        return where

    glimpse_all = np.ones((4, B, h, w))
    obs = sum(prune._st_write(glimpse_all[i], rows([i])[0], (H, W)) for i in (0, 1, 2)) * mult       # three blobs
    cur = dict(what=rng.normal(size=(T, B, A)) * 0.1, where=rows([0, 3]), glimpse=np.ones((T, B, h * w)), score=np.full((T, B), 0.5))
    n = np.array([2, 1, 0])                                        # start: blob 0 and a spurious blob 3
    prior = np.array([0.2, 0.3, 0.5])
    src, objectives, starts, sources = None, [], [], []
    for r, blob in enumerate((1, 2)):                              # round r "proposes" a blob the scene holds
        res, energy = propose.reference_residual(cur["glimpse"].reshape(T, B, h, w), cur["where"], n, obs, mult)
        assert (res >= 0).all() and (res <= 1).all()
        prop = dict(prop_what=rng.normal(size=(T, B, A)) * 0.1, prop_where=rows([blob, blob]), prop_glimpse=np.ones((T, B, h * w)),
                    prop_score=np.full((T, B), 0.25))
        pool = propose.reference_pool(**cur, n=n, **prop, prior=prior, proposals=P, round=r, source_in=src)
        rec = prune.reference_score(pool["glimpse"].reshape(T + P, B, h, w), pool["where"], pool["presence"], obs, mult, std, True)
        sel = prune.reference_select(pool["what"], pool["where"], pool["glimpse"], pool["score"], pool["presence"], None, PRIORS,
                                     pool["prior"], 1, True, rec)
        assert (sel["num_objects"] <= T).all()
        src = propose.reference_source(pool["source"], sel["kept_step"])
        sources.append((src.copy(), sel["num_objects"].copy()))
        objectives.append(sel["objective"]); starts.append(sel["objective_start"])
        cur = {k: sel[k][:T] for k in ("what", "where", "glimpse", "score")}
        n = sel["num_objects"]
    assert np.array_equal(starts[1], objectives[0])                # bit for bit
    assert (objectives[0] >= starts[0]).all() and (objectives[1] >= objectives[0]).all()
    assert (objectives[0] > starts[0]).any()
    # image 0 started with blob 0 + the spurious blob: round 0 swaps the spurious one for proposal 0 of round 0 (source T + 0);
    # image 2 started empty: every pool row is a candidate, it gains start row 0 and that proposal
    src0, n0 = sources[0]
    assert src0[:2, 0].tolist() == [0, T + 0] and n0[0] == 2 and src0[:2, 2].tolist() == [0, T + 0] and n0[2] == 2
    assert n[0] == 2 and set(sources[1][0][:2, 0].tolist()) <= {0, T + 0, T + P}


# ---- 6. the header and the binding --------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_binding_matches():
    from attend_infer_repeat_amd import _lib
    text = open(HEADER).read()
    for name, n_args in (("air_propose_residual", 17), ("air_propose_pool", 26), ("air_propose_source", 6)):
        m = re.search(r"AIR_ENGINE_API int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5
    from attend_infer_repeat_amd import build
    assert "propose_kernels.hip" in build.SOURCES
