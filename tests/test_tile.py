"""GPU tests of tiled scene parsing (attend_infer_repeat_amd/tile.py, csrc/tile_kernels.hip): air_tile_gather against
tile.reference_gather bit for bit, air_tile_merge against tile.reference_merge on crafted fp32 rows (margins asserted), then
TiledSceneParser: the identity at scene == canvas, the composition gather -> provider -> merge -> read-out against the host reference
and the existing read-out entries, a planted scene, graph replay against eager, the module's behaviour, scoring and the surface.

Bars.  Everything the merge decides is compared exactly, on inputs whose decisions are not within rounding of flipping: every box
centre at least CENTRE_MARGIN pixels from a cell boundary, every cross-window IoU at least IOU_MARGIN from the threshold (float64
arithmetic on numbers of order 1 .. 100: rounding differences between two float64 evaluations are below 1e-13).  Copies are compared
by bits, the lifted `where` within one fp32 ulp of the float64 reference rounded to fp32.  The planted scene's rendering is the kind of
number a canvas is: test_engine.py's OUT_TOL / OUT_L2."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from oracle import air_oracle as O
from test_engine import OUT_L2, OUT_TOL, l2_err, rel_err
from test_parse import MASK_THRESHOLD, SENTINEL_F, SENTINEL_I, _mnist_air, _train_state, e2e_case, engine_config, make_parser, \
    run_objects, run_render
from test_tile_host import build_rows, merge_margins, overflow_case, scene_row, unlift

from attend_infer_repeat_amd import prune, tile

pytestmark = pytest.mark.gpu

CENTRE_MARGIN, IOU_MARGIN = 1e-6, 1e-9
dev_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


# ---- 1. air_tile_gather ---------------------------------------------------------------------------------------------------------------
GATHER_CASES = {"clamped_unaligned": ((7, 9), (5, 6), (2, 3), 3), "one_window": ((5, 6), (5, 6), (5, 6), 2),
                "aligned": ((12, 16), (8, 8), (4, 4), 2), "stride_1": ((9, 13), (4, 5), (1, 1), 1),
                "100_50_25": ((100, 100), (50, 50), (25, 25), 2)}


def run_gather(scenes, img, stride, tail=64, **kw):
    """air_tile_gather alone (current stream); a sentinel fills the output and `tail` floats behind it"""
    from attend_infer_repeat_amd import hip as Hh
    S, Hs, Ws = scenes.shape
    (H, W), (sy, sx) = img, stride
    oy, ox = tile.window_origins((Hs, Ws), img, stride)
    n = S * len(oy) * len(ox) * H * W
    out = torch.full((n + tail,), SENTINEL_F, device="cuda")
    a = dict(src=Hh._p(scenes), S=S, Hs=Hs, Ws=Ws, H=H, W=W, sy=sy, sx=sx, out=Hh._p(out))
    a.update(kw)
    st = Hh.lib().air_tile_gather(a["src"], a["S"], a["Hs"], a["Ws"], a["H"], a["W"], a["sy"], a["sx"], a["out"], Hh._stream())
    torch.cuda.synchronize()
    return st, out[:n].view(-1, H * W), out[n:]


@pytest.mark.parametrize("name", sorted(GATHER_CASES))
def test_gather_is_the_reference_bit_for_bit(gpu_device, name):
    scene, img, stride, S = GATHER_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    scenes = rng.normal(size=(S,) + scene).astype(np.float32)
    scenes[0, 0, 0], scenes[-1, -1, -1] = np.nan, -0.0
    st, got, tail = run_gather(dev_t(scenes), img, stride)
    assert st == 0
    want = tile.reference_gather(scenes, img, stride)
    assert got.shape == want.shape and np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert (tail == SENTINEL_F).all()


def test_gather_from_an_unaligned_base_takes_the_word_path(gpu_device):
    scene, img, stride, S = GATHER_CASES["aligned"]
    rng = np.random.default_rng(4)
    scenes = rng.normal(size=(S,) + scene).astype(np.float32)
    flat = torch.zeros(scenes.size + 1, device="cuda")
    flat[1:] = dev_t(scenes).reshape(-1)
    st, got, tail = run_gather(flat[1:].view(scenes.shape), img, stride)
    assert st == 0 and np.array_equal(bits(got.cpu().numpy()), bits(tile.reference_gather(scenes, img, stride)))
    assert (tail == SENTINEL_F).all()


def test_gather_argument_checks_write_nothing(gpu_device):
    scenes = torch.zeros((2, 12, 16), device="cuda")
    for kw, code in ((dict(src=None), -1), (dict(out=None), -1), (dict(Hs=7), -2), (dict(Ws=7), -2), (dict(sy=0), -2),
                     (dict(sy=9), -2), (dict(sx=0), -2), (dict(sx=9), -2), (dict(S=0), -2), (dict(H=1, sy=1), -2),
                     (dict(W=1, sx=1), -2)):
        st, got, tail = run_gather(scenes, (8, 8), (4, 4), **kw)
        assert st == code, kw
        assert (got == SENTINEL_F).all() and (tail == SENTINEL_F).all()


# ---- 2. air_tile_merge ----------------------------------------------------------------------------------------------------------------
IMG = (8, 10)
GEOMETRY = {1: ((8, 10), (4, 5)), 4: ((12, 15), (4, 5)), 9: ((16, 20), (4, 5)), 64: ((22, 31), (2, 3))}      # Nw -> scene, stride


def crafted_rows(T, A, G, Nw, S, seed, tie=False):
    """random provider rows around a few true objects per scene: every window that sees an object's centre reports it with a jitter
    (so cells, duplicates and truncated sightings all occur), plus clutter; redrawn until the margins hold"""
    scene, stride = GEOMETRY[Nw]
    oy, ox = tile.window_origins(scene, IMG, stride)
    nx = len(ox)
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        sightings = []
        for s in range(S):
            seen = np.zeros(Nw, np.int64)
            objs = [(rng.uniform(1, scene[1] - 1), rng.uniform(1, scene[0] - 1), rng.uniform(2, 5), rng.uniform(2, 5))
                    for _ in range(rng.integers(0, 2 + Nw // 2))]
            (ylo, yhi), (xlo, xhi) = tile.cell_bounds(oy, IMG[0]), tile.cell_bounds(ox, IMG[1])
            for _ in range(2 if nx > 1 else 0):                    # a pair that straddles a cell boundary: each window owns its sighting
                i, j = int(rng.integers(0, len(oy))), int(rng.integers(0, nx - 1))
                cy = rng.uniform(max(ylo[i], 0.0) + 0.5, min(yhi[i], scene[0]) - 0.5)
                d, (bw, bh) = rng.uniform(0.05, 0.4), rng.uniform(2, 5, 2)
                shrink = 1.0 if rng.uniform() < 0.7 else 0.4       # (sometimes too different to be the same object)
                for v, cx, k in ((i * nx + j, xhi[j] - d, 1.0), (i * nx + j + 1, xhi[j] + d, shrink)):
                    if seen[v] < T:
                        sightings.append((s, v, cx, cy, bw * k, bh * k, rng.uniform()))
                        seen[v] += 1
            for v in rng.permutation(Nw):
                i, j = divmod(int(v), nx)
                for (cx, cy, bw, bh) in objs:
                    if seen[v] < T and ox[j] <= cx < ox[j] + IMG[1] and oy[i] <= cy < oy[i] + IMG[0] and rng.uniform() < 0.8:
                        jit = rng.normal(size=4) * 0.15
                        sightings.append((s, int(v), cx + jit[0], cy + jit[1], bw + jit[2], bh + jit[3], rng.uniform()))
                        seen[v] += 1
                if seen[v] < T and rng.uniform() < 0.3:            # clutter anywhere in the window
                    sightings.append((s, int(v), ox[j] + rng.uniform(0, IMG[1]), oy[i] + rng.uniform(0, IMG[0]), 3.0, 3.0,
                                      rng.uniform()))
                    seen[v] += 1
        what, where, glimpse, score, n, cands = build_rows(sightings, scene, IMG, stride, T, S=S, A=A, G=G, seed=seed)
        if tie and len(sightings) >= 2:                            # planted exact ties: the first sighting's score, all over scene 0
            first = sightings[0]
            score[:, :Nw] = np.float32(first[6])
        centre, iou, ties = merge_margins(where, score, n, scene, IMG, stride)
        if (centre >= CENTRE_MARGIN).all() and (iou >= IOU_MARGIN).all() and (tie or ties.sum() == 0):
            return dict(what=what, where=where, glimpse=glimpse, score=score, n=n, scene=scene, stride=stride, T=T, S=S, Nw=Nw)
    raise AssertionError("no crafted case within the margins")


def run_merge(case, iou_merge=0.5, img=IMG, **kw):
    """air_tile_merge alone (current stream); every output starts as a sentinel fill"""
    from attend_infer_repeat_amd import hip as Hh
    T, R, A = case["what"].shape
    G = case["glimpse"].shape[2]
    (Hs, Ws), (sy, sx), S, Nw = case["scene"], case["stride"], case["S"], case["Nw"]
    Nc, C = Nw * T, min(Nw * T, 32)
    ff = lambda *s: torch.full(s, SENTINEL_F, device="cuda")
    fi = lambda *s: torch.full(s, SENTINEL_I, dtype=torch.int32, device="cuda")
    d = {k: dev_t(case[k]) for k in ("what", "where", "glimpse", "score")}
    d["n"] = dev_t(case["n"].astype(np.int32))
    out = dict(what=ff(C, S, A), where=ff(C, S, 4), glimpse=ff(C, S, G), score_src=ff(C, S), kept_cand=fi(C, S), num_objects=fi(S),
               cand_state=torch.full((S, Nc), 99, dtype=torch.int8, device="cuda"), dup_of=fi(S, Nc), merge_counts=fi(S, 6))
    p = Hh._p
    a = dict(T=T, S=S, Hs=Hs, Ws=Ws, H=img[0], W=img[1], sy=sy, sx=sx, what=p(d["what"]), where=p(d["where"]),
             where_out=p(out["where"]), cand_state=p(out["cand_state"]))
    a.update(kw)
    st = Hh.lib().air_tile_merge(a["what"], a["where"], p(d["glimpse"]), p(d["score"]), p(d["n"]), a["T"], a["S"], A, G, a["Hs"], a["Ws"],
                                 a["H"], a["W"], a["sy"], a["sx"], float(iou_merge), p(out["what"]), a["where_out"], p(out["glimpse"]),
                                 p(out["score_src"]), p(out["kept_cand"]), p(out["num_objects"]), a["cand_state"], p(out["dup_of"]),
                                 p(out["merge_counts"]), Hh._stream())
    torch.cuda.synchronize()
    return st, {k: v.cpu().numpy() for k, v in out.items()}


def ulp_distance(a, b):
    """distance in fp32 units in the last place between two finite arrays (sign-magnitude to two's complement first)"""
    f = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return np.abs(f(np.ascontiguousarray(a, np.float32)) - f(np.ascontiguousarray(b, np.float32)))


def check_merge(case, got, ref, worst=None):
    for k in ("cand_state", "dup_of", "merge_counts", "num_objects", "kept_cand"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    S, n = case["S"], ref["num_objects"]
    for s in range(S):
        for k in ("what", "glimpse", "score_src"):
            assert np.array_equal(bits(got[k][:n[s], s]), bits(ref[k][:n[s], s])), (k, s)
            assert (got[k][n[s]:, s] == SENTINEL_F).all(), (k, s)
        assert (got["where"][n[s]:, s] == SENTINEL_F).all()
        if n[s]:
            d = int(ulp_distance(got["where"][:n[s], s], ref["where"][:n[s], s]).max())
            if worst is not None:
                worst.append(d)
            assert d <= 1, (s, d)


MERGE_PARAMS = [(T, A, G, Nw, S) for T in (1, 3) for (A, G) in ((50, 400), (7, 9), (12, 16)) for Nw in (1, 4, 9) for S in (1, 5)] + \
    [(4, 12, 16, 64, 2), (3, 7, 9, 64, 2)]


@pytest.mark.parametrize("T,A,G,Nw,S", MERGE_PARAMS)
def test_merge_is_the_reference(gpu_device, T, A, G, Nw, S):
    case = crafted_rows(T, A, G, Nw, S, seed=T + A + Nw + S)
    centre, iou, ties = merge_margins(case["where"], case["score"], case["n"], case["scene"], IMG, case["stride"])
    assert (centre >= CENTRE_MARGIN).all() and (iou >= IOU_MARGIN).all() and ties.sum() == 0
    st, got = run_merge(case)
    assert st == 0
    ref = tile.reference_merge(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["scene"], IMG, case["stride"])
    worst = []
    check_merge(case, got, ref, worst)
    print("lifted where, worst distance from the rounded float64 reference: %d ulp" % max(worst + [0]))
    if Nw > 1 and S > 1:
        assert ref["merge_counts"][:, tile.KEPT].sum() > 0


def test_merge_finds_duplicates_somewhere(gpu_device):
    """the crafted cases do contain double sightings (state 3), or the parametrised test above would prove little"""
    total = np.zeros(6, np.int64)
    for (T, A, G, Nw, S) in [(3, 7, 9, 9, 5), (3, 12, 16, 4, 5), (4, 12, 16, 64, 2)]:
        case = crafted_rows(T, A, G, Nw, S, seed=T + A + Nw + S)
        total += run_merge(case)[1]["merge_counts"].sum(0)
    assert total[tile.DUPLICATE] > 0 and total[tile.KEPT] > 0 and total[tile.NOT_OWNED] > 0 and total[tile.ABSENT] > 0


def test_merge_planted_ties_go_to_the_lower_candidate(gpu_device):
    case = crafted_rows(3, 12, 16, 9, 2, seed=77, tie=True)
    _, _, ties = merge_margins(case["where"], case["score"], case["n"], case["scene"], IMG, case["stride"])
    assert ties[0] > 0
    st, got = run_merge(case)
    ref = tile.reference_merge(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["scene"], IMG, case["stride"])
    assert st == 0
    check_merge(case, got, ref)
    # and the hand case of the host tests: the same score in two windows
    scene, stride = (10, 20), (5, 5)
    what, where, glimpse, score, n, cands = build_rows([(0, 1, 7.6, 5.0, 4.0, 4.0, 0.5), (0, 0, 7.4, 5.0, 4.0, 4.0, 0.5)], scene, (10, 10),
                                                       stride, 2)
    hand = dict(what=what, where=where, glimpse=glimpse, score=score, n=n, scene=scene, stride=stride, T=2, S=1, Nw=3)
    st, got = run_merge(hand, img=(10, 10))
    assert st == 0 and got["cand_state"][0, [0, 2]].tolist() == [tile.KEPT, tile.DUPLICATE] and got["dup_of"][0, 2] == 0


def test_merge_nonfinite_rows_overflow_and_all_absent(gpu_device):
    case = crafted_rows(3, 7, 9, 9, 5, seed=5)
    rows = [(t, r) for r in range(case["n"].size) for t in range(case["n"][r])]
    assert len(rows) >= 6
    for q, (k, bad) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan))):
        t, r = rows[q]
        case["where"][t, r, k] = bad
    case["score"][rows[4]] = np.nan
    case["score"][rows[5]] = np.inf
    st, got = run_merge(case)
    ref = tile.reference_merge(case["what"], case["where"], case["glimpse"], case["score"], case["n"], case["scene"], IMG, case["stride"])
    assert st == 0 and ref["merge_counts"][:, tile.NONFINITE].sum() == 6
    check_merge(case, got, ref)
    # 40 owned candidates that overlap nothing: 32 kept, the 8 lowest scores overflow
    sightings, scene, img, stride, T, scores = overflow_case()
    what, where, glimpse, score, n, cands = build_rows(sightings, scene, img, stride, T, A=12, G=16)
    over = dict(what=what, where=where, glimpse=glimpse, score=score, n=n, scene=scene, stride=stride, T=T, S=1, Nw=10)
    st, got = run_merge(over, img=img)
    ref = tile.reference_merge(what, where, glimpse, score, n, scene, img, stride)
    assert st == 0 and got["merge_counts"][0].tolist() == [0, 32, 0, 0, 8, 0]
    check_merge(over, got, ref)
    assert sorted(np.flatnonzero(got["cand_state"][0] == tile.OVERFLOW).tolist()) == sorted(np.argsort(scores)[:8].tolist())
    # nothing present
    case = crafted_rows(3, 7, 9, 4, 5, seed=6)
    case["n"][:] = 0
    st, got = run_merge(case)
    assert st == 0 and (got["num_objects"] == 0).all() and (got["cand_state"] == 0).all() and (got["kept_cand"] == -1).all()
    assert (got["what"] == SENTINEL_F).all() and (got["where"] == SENTINEL_F).all() and (got["merge_counts"][:, 0] == 12).all()


def test_merge_argument_checks_write_nothing(gpu_device):
    case = crafted_rows(3, 7, 9, 4, 2, seed=8)
    from attend_infer_repeat_amd import hip as Hh
    off = torch.zeros(3 * 8 * 4 + 1, device="cuda")
    for kw, code in ((dict(what=None), -1), (dict(cand_state=None), -1), (dict(T=0), -2), (dict(T=33), -2), (dict(Hs=7), -2),
                     (dict(sy=0), -2), (dict(sx=11), -2), (dict(S=0), -2), (dict(H=1, sy=1), -2), (dict(Hs=64, Ws=80, sy=1, sx=1), -2),
                     (dict(where=Hh._p(off[1:])), -3)):
        st, got = run_merge(case, **kw)
        assert st == code, kw
        assert (got["what"] == SENTINEL_F).all() and (got["num_objects"] == SENTINEL_I).all() and (got["cand_state"] == 99).all()


def test_relabel_takes_32_rows(gpu_device):
    from attend_infer_repeat_amd import hip as Hh
    C, S = 32, 5
    rng = np.random.default_rng(2)
    n = np.array([0, 32, 7, 1, 40])
    nc = np.minimum(n, C)
    offsets = np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)
    src = rng.uniform(size=(C, S)).astype(np.float32)
    kept = rng.integers(0, 256, (C, S)).astype(np.int32)
    d = dict(score=torch.full((C, S), SENTINEL_F).cuda(), obj_score=torch.full((C * S,), SENTINEL_F).cuda(),
             obj_step=torch.full((C * S,), SENTINEL_I, dtype=torch.int32).cuda())
    p = Hh._p
    d.update(src=dev_t(src), kept=dev_t(kept), n=dev_t(n.astype(np.int32)), offsets=dev_t(offsets))
    st = Hh.lib().air_tile_relabel(p(d["src"]), p(d["kept"]), p(d["n"]), p(d["offsets"]), C, S, p(d["score"]), p(d["obj_score"]),
                                   p(d["obj_step"]), Hh._stream())
    torch.cuda.synchronize()
    assert st == 0
    want_score, want_os = np.full((C, S), SENTINEL_F, np.float32), np.full(C * S, SENTINEL_F, np.float32)
    want_step = np.full(C * S, SENTINEL_I, np.int32)
    for s in range(S):
        want_score[:nc[s], s] = src[:nc[s], s]
        want_os[offsets[s]:offsets[s] + nc[s]] = src[:nc[s], s]
        want_step[offsets[s]:offsets[s] + nc[s]] = kept[:nc[s], s]
    assert np.array_equal(d["score"].cpu().numpy(), want_score) and np.array_equal(d["obj_score"].cpu().numpy(), want_os)
    assert np.array_equal(d["obj_step"].cpu().numpy(), want_step)


# ---- 3. identity ----------------------------------------------------------------------------------------------------------------------
TABLE = ("obj_image", "obj_step", "obj_box", "obj_score", "obj_where", "obj_what")


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("name", ["tiny", "mnist_b8"])
def test_one_window_is_the_providers_parse(gpu_device, name, given):
    """given: the provider is handed counts 0 .. T (further arguments of parse() go to it unchanged), so that every row count occurs
    whatever the random weights' own count head says"""
    from attend_infer_repeat_amd.tile import TiledSceneParser
    ocfg, B, params, obs = e2e_case(name)
    ps = make_parser(ocfg, B, params)
    tp = TiledSceneParser(ps, ocfg.img_size)
    assert (tp.T, tp.R, tp.n_windows) == (ps.T, B, 1) and tp.engine is ps.engine
    counts = (torch.arange(B, dtype=torch.int32) % (ps.T + 1)).cuda() if given else None
    out = tp.parse(obs.cuda(), counts)
    tp.synchronize()
    got = {k: v.clone() for k, v in out.items()}
    base = ps.parse(obs.cuda(), counts)
    ps.synchronize()
    n = base["num_objects"].cpu().numpy()
    assert torch.equal(got["num_objects"], base["num_objects"]) and (not given or n.tolist() == counts.tolist())
    for k in ("presence", "owner", "reconstruction", "area", "rec", "offsets"):
        assert torch.equal(got[k], base[k]), k
    for k in ("where", "what", "glimpse", "score", "boxes"):       # (rows beyond the count are not written by the merge)
        for r in range(B):
            assert torch.equal(got[k][:n[r], r], base[k][:n[r], r]), (k, r)
    rows = int(base["offsets"][-1])
    for k in TABLE:
        assert torch.equal(got[k][:rows], base[k][:rows]), k
    assert torch.equal(got["windows"].reshape(B, -1), obs.cuda().reshape(B, -1))
    assert torch.equal(got["window_num_objects"].reshape(-1), base["num_objects"])
    assert torch.equal(got["window_count_prob"].reshape(-1), base["count_prob"]) and "count_prob" not in got
    assert got["merge_counts"][:, [2, 3, 4, 5]].sum() == 0


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------
def make_tiled(name, provider="scene", S=8, capture=False, scale=2):
    from attend_infer_repeat_amd.prune import ParsePruner
    from attend_infer_repeat_amd.tile import TiledSceneParser
    ocfg, _, params, _ = e2e_case(name)
    scene = (scale * ocfg.img_size[0], scale * ocfg.img_size[1])
    _, _, (ny, nx) = tile.check_geometry(scene, ocfg.img_size)
    ps = make_parser(ocfg, S * ny * nx, params)
    pr = ps if provider == "scene" else ParsePruner(ps, "present")
    tp = TiledSceneParser(pr, scene)
    if capture:
        ps.capture()
        if pr is not ps:
            pr.capture()
        tp.capture()
    return ocfg, tp, pr, scene


def scenes_for(ocfg, scene, S, seed):
    return O.synthetic_batch(dataclasses.replace(ocfg, img_size=scene), S, seed=seed, max_objects=4)[0]


@pytest.mark.parametrize("name,provider", [("tiny", "scene"), ("rect_t5", "scene"), ("tiny", "prune"), ("rect_t5", "prune")])
def test_module_is_gather_provider_merge_readout(gpu_device, name, provider):
    S = 8
    ocfg, tp, pr, scene = make_tiled(name, provider, S)
    img, crop, T = tuple(ocfg.img_size), tuple(ocfg.crop_size), ocfg.max_steps
    scenes = scenes_for(ocfg, scene, S, seed=21)
    counts = torch.from_numpy(np.random.default_rng(9).integers(0, T + 1, pr.R).astype(np.int32)).cuda()      # (random weights: the
    out = tp.parse(scenes.cuda(), counts)                          #  count head's own answer may be 0 everywhere)
    tp.synchronize()
    got = {k: v.clone() for k, v in out.items()}
    # the same through public pieces: numpy windows, the provider's own parse, the host merge, the existing read-out entries
    windows = tile.reference_gather(scenes.numpy(), img)
    assert np.array_equal(bits(got["windows"].cpu().numpy().reshape(windows.shape)), bits(windows))
    base = pr.parse(dev_t(windows).view(-1, *img), counts)
    pr.synchronize()
    rows = {k: base[k].cpu().numpy().reshape(T, pr.R, -1) for k in ("what", "where", "glimpse")}
    score, n_in = base["score"].cpu().numpy(), base["num_objects"].cpu().numpy()
    assert n_in.max() > 0 or provider == "prune"                   # (the subset search may empty every window of a random model)
    ref = tile.reference_merge(rows["what"], rows["where"], rows["glimpse"], score, n_in, scene, img)
    centre, iou, ties = merge_margins(rows["where"], score, n_in, scene, img, None)
    safe = (centre >= CENTRE_MARGIN) & (iou >= IOU_MARGIN)         # (equal fp32 scores are no rounding matter: the lower id wins)
    print("scenes inside the margins: %d of %d; kept %s" % (safe.sum(), S, ref["num_objects"].tolist()))
    assert (~safe).sum() <= S // 8
    for k in ("cand_state", "dup_of", "merge_counts"):
        assert np.array_equal(got[k].cpu().numpy()[safe], ref[k][safe]), k
    assert np.array_equal(got["num_objects"].cpu().numpy()[safe], ref["num_objects"][safe])
    assert np.array_equal(got["kept_cand"].cpu().numpy()[:, safe], ref["kept_cand"][:, safe])
    # the read-out on the module's own compacted rows (every scene), and on the reference's rows where the decisions are safe
    n_dev = got["num_objects"]
    obj = run_objects(None, n_dev, got["where"], got["what"], *scene)
    ren = run_render(got["glimpse"].reshape(tp.T, S, -1), got["where"], obj["presence"], scenes.cuda(), ocfg.output_multiplier,
                     ocfg.output_std, scene, crop, layers=False)
    for k in ("presence", "boxes", "offsets"):
        assert torch.equal(got[k], obj[k]), k
    for k in ("reconstruction", "owner", "area", "rec"):
        assert torch.equal(got[k], ren[k]), k
    nrows = int(obj["offsets"][-1])
    for k in ("obj_image", "obj_box", "obj_where", "obj_what"):
        assert torch.equal(got[k][:nrows], obj[k][:nrows]), k
    n = ref["num_objects"]
    step = np.concatenate([ref["kept_cand"][:n[s], s] for s in range(S)])
    osc = np.concatenate([ref["score_src"][:n[s], s] for s in range(S)])
    if safe.all():
        assert np.array_equal(got["obj_step"].cpu().numpy()[:nrows], step)
        assert np.array_equal(bits(got["obj_score"].cpu().numpy()[:nrows]), bits(osc))
    for s in np.flatnonzero(safe):
        for k, r in (("what", ref["what"]), ("glimpse", ref["glimpse"].reshape(tp.T, S, *crop)), ("score", ref["score_src"])):
            assert np.array_equal(bits(got[k].cpu().numpy()[:n[s], s]), bits(r[:n[s], s])), (k, s)
        if n[s]:
            assert ulp_distance(got["where"].cpu().numpy()[:n[s], s], ref["where"][:n[s], s]).max() <= 1
    assert ref["num_objects"].max() > 0 or provider == "prune"


# ---- 5. planted scene -----------------------------------------------------------------------------------------------------------------
def test_planted_scene_through_the_module(gpu_device):
    """scene 0: an object in the overlap of windows 0 and 1 that each of them places on its own side of the cell boundary (a double
    sighting: state 3 for the lower score), an object whole in window 4 alone, and window 0's truncated sighting of something whose
    centre lies in window 1's cell (state 2).  Scene 1: ONE scene-frame row given to windows 0 and 1 as its exact inverse lift -- by
    the half-open cells the two share a centre and so an owner: kept once, the other sighting is state 2, never a duplicate."""
    S = 2
    ocfg, tp, ps, scene = make_tiled("rect_t5", "scene", S)
    img, crop, T = tuple(ocfg.img_size), tuple(ocfg.crop_size), ocfg.max_steps         # 28 x 36 in 56 x 72: ox = 0, 18, 36; oy = 0, 14, 28
    scenes = scenes_for(ocfg, scene, S, seed=3)
    tp.stage(scenes.cuda())
    tp.run_segments("gather")
    tp.run_provider()
    tp.synchronize()
    eng = ps.engine
    oy, ox = tile.window_origins(scene, img)
    A_left, A_right = scene_row(26.8, 8.0, 10.0, 9.0, scene), scene_row(27.2, 8.0, 10.0, 9.0, scene)      # the boundary is at 27
    B_row = scene_row(40.0, 30.0, 12.0, 10.0, scene)                # whole in window 4 (18 .. 54 x 14 .. 42), its cell
    trunc = scene_row(31.0, 20.0, 8.0, 8.0, scene)                  # window 0 sees it cut at x = 36; the centre is window 1's (and row 0's)
    E_row = scene_row(30.0, 9.0, 10.0, 8.0, scene)
    plant = {(0, 0): [(A_left, 0.9), (trunc, 0.95)], (0, 1): [(A_right, 0.6)], (0, 4): [(B_row, 0.7)],
             (1, 0): [(E_row, 0.9)], (1, 1): [(E_row, 0.5)]}
    where, score = eng.where.cpu().numpy().copy(), ps.score.cpu().numpy().copy()
    n = np.zeros(ps.R, np.int32)
    for (s, v), objs in plant.items():
        r = s * 9 + v
        for t, (row, sc) in enumerate(objs):
            where[t, r] = unlift(row, scene, img, (oy[v // 3], ox[v % 3])).astype(np.float32)
            score[t, r] = sc
        n[r] = len(objs)
    eng.where.copy_(dev_t(where))
    ps.score.copy_(dev_t(score))
    ps.num_objects.copy_(dev_t(n))
    torch.cuda.synchronize()
    tp.run_segments("merge", "objects", "relabel", "render", "rec_sum")
    tp.synchronize()
    out = tp.result()
    state, dup = out["cand_state"].cpu().numpy(), out["dup_of"].cpu().numpy()
    assert out["num_objects"].tolist() == [2, 1]
    assert out["kept_cand"][:2, 0].tolist() == [0, 4 * T] and out["kept_cand"][0, 1].item() == 1 * T      # the owning windows
    assert state[0, 0] == tile.KEPT and state[0, 1] == tile.NOT_OWNED and state[0, T] == tile.DUPLICATE and dup[0, T] == 0
    assert state[0, 4 * T] == tile.KEPT and state[1, 0] == tile.NOT_OWNED and state[1, T] == tile.KEPT
    assert out["merge_counts"].tolist() == [[9 * T - 4, 2, 1, 1, 0, 0], [9 * T - 2, 1, 1, 0, 0, 0]]
    assert out["obj_step"][:3].tolist() == [0, 4 * T, T] and out["obj_score"][:3].tolist() == [np.float32(0.9), np.float32(0.7),
                                                                                               np.float32(0.5)]
    # the rendering: the kept rows' glimpses written at the scene-frame rows, in float64
    glimpse = eng.gd.out[-1].cpu().numpy().reshape(T, ps.R, *crop).astype(np.float64)
    want = np.zeros((S,) + scene)
    want[0] = prune._st_write(glimpse[0, 0][None], A_left[None], scene)[0] + prune._st_write(glimpse[0, 4][None], B_row[None], scene)[0]
    want[1] = prune._st_write(glimpse[0, 9 + 1][None], E_row[None], scene)[0]
    want *= ocfg.output_multiplier
    got = out["reconstruction"]
    e, e2 = rel_err(got, torch.from_numpy(want)), l2_err(got, torch.from_numpy(want))
    print("planted scene rendering: max %.3g, l2 %.3g" % (e, e2))
    assert np.abs(want).max() > 0 and e < OUT_TOL and e2 < OUT_L2
    # the scene boxes are attention_box of the scene-frame rows
    boxes = out["boxes"].cpu().numpy()
    assert np.allclose(boxes[0, 0], [21.8, 3.5, 10.0, 9.0], atol=1e-4) and np.allclose(boxes[1, 0], [34.0, 25.0, 12.0, 10.0], atol=1e-4)


# ---- 6. graph and module behaviour ------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_nothing_leaks(gpu_device):
    S = 4
    ocfg, eager, _, scene = make_tiled("rect_t5", "scene", S)
    _, graph, _, _ = make_tiled("rect_t5", "scene", S, capture=True)
    full, empty = scenes_for(ocfg, scene, S, seed=31), torch.zeros((S,) + scene)
    other = scenes_for(ocfg, scene, S, seed=32)
    counts = []
    for scenes in (full, other, empty, full):
        a, b = eager.parse(scenes.cuda()), graph.parse(scenes.cuda())
        eager.synchronize(); graph.synchronize()
        assert set(a) == set(b)
        n = b["num_objects"].cpu().numpy()
        for k in a:
            if k in ("what", "where", "glimpse", "score", "boxes") or k in TABLE:
                continue                                           # rows beyond the count are whatever an earlier call left
            assert torch.equal(a[k], b[k]), k
        for k in ("what", "where", "glimpse", "score", "boxes"):
            for s in range(S):
                assert torch.equal(a[k][:n[s], s], b[k][:n[s], s]), (k, s)
        rows = int(b["offsets"][-1])
        for k in TABLE:
            assert torch.equal(a[k][:rows], b[k][:rows]), k
        counts.append((n.copy(), b["reconstruction"].clone(), b["owner"].clone()))
    assert counts[0][0].sum() > 0
    # fewer objects after more: the empty scenes' result does not remember the full ones
    first = {k: v.clone() for k, v in graph.parse(full.cuda()).items()}
    again = {k: v.clone() for k, v in graph.parse(full.cuda()).items()}
    graph.synchronize()
    assert all(torch.equal(first[k], again[k]) for k in first if k not in ("score", "obj_score"))      # (NaN beyond the count)
    assert torch.equal(counts[0][1], counts[3][1]) and torch.equal(counts[0][2], counts[3][2]) and (counts[0][0] == counts[3][0]).all()
    fresh = make_tiled("rect_t5", "scene", S)[1]
    lone = fresh.parse(empty.cuda())
    fresh.synchronize()
    assert torch.equal(lone["num_objects"], torch.from_numpy(counts[2][0]).cuda())
    assert torch.equal(lone["reconstruction"], counts[2][1]) and torch.equal(lone["owner"], counts[2][2])
    assert {k: v for k, v in graph.launch_count().items() if k != "parser"} == {
        "tile_gather": 1, "tile_merge": 1, "parse_objects": 1, "tile_relabel": 1, "parse_render": 1, "rec_sum": 1}
    assert list(graph.segments) == ["gather", "merge", "objects", "relabel", "render", "rec_sum"]
    graph.release_graphs()


def test_update_config_rebuilds_the_launch_list(gpu_device):
    S = 2
    ocfg, tp, ps, scene = make_tiled("rect_t5", "scene", S, capture=True)
    scenes = scenes_for(ocfg, scene, S, seed=31).cuda()
    a = {k: v.clone() for k, v in tp.parse(scenes).items()}
    assert tp.update_config(output_multiplier=2 * ocfg.output_multiplier) and tp._graph is not None
    b = {k: v.clone() for k, v in tp.parse(scenes).items()}
    tp.synchronize()
    assert a["num_objects"].sum() > 0 and torch.equal(a["kept_cand"], b["kept_cand"])
    assert torch.equal(b["reconstruction"], 2 * a["reconstruction"]) and not torch.equal(a["rec"], b["rec"])
    ps.update_config(output_multiplier=ocfg.output_multiplier)      # behind the tiled parser's back: noticed at the next call
    c = tp.parse(scenes)
    tp.synchronize()
    assert torch.equal(c["reconstruction"], a["reconstruction"]) and torch.equal(c["rec"], a["rec"])
    tp.release_graphs()


def test_refusals(gpu_device):
    import types
    from attend_infer_repeat_amd.tile import TiledSceneParser
    ocfg, B, params, _ = e2e_case("tiny")
    ps = make_parser(ocfg, 10, params)
    with pytest.raises(ValueError, match="multiple"):
        TiledSceneParser(ps, (6, 6))                                # 16 windows, 10 rows
    with pytest.raises(ValueError, match="smaller"):
        TiledSceneParser(ps, (2, 6))
    with pytest.raises(ValueError, match="ParticleParser"):
        TiledSceneParser(types.SimpleNamespace(KIND="particle", engine=ps.engine, R=10, T=3), ocfg.img_size)     # a particle provider
    tp = TiledSceneParser(ps, ocfg.img_size)
    with pytest.raises(ValueError, match="scenes"):
        tp.parse(torch.zeros(3, 3, 3).cuda())


def test_parse_tiled_on_the_model_does_not_disturb_training(gpu_device):
    from attend_infer_repeat_amd.data import create_multi_mnist
    B = 8
    air, ts, x, y = _mnist_air(B)
    twin, ts_twin, _, _ = _mnist_air(B)
    for _ in range(2):
        ts(); ts_twin()
    rng = np.random.default_rng(0)
    scenes = torch.from_numpy(rng.uniform(size=(2, 100, 120)).astype(np.float32) * (rng.uniform(size=(2, 100, 120)) > 0.9)).cuda()
    before, obs_before = _train_state(air._engine), air.obs
    out = air.parse_tiled(scenes)
    after = _train_state(air._engine)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert air.obs is obs_before and air._engine.global_step == 2
    C, S, T = 32, 2, 3
    shapes = {"num_objects": (S,), "presence": (C, S), "score": (C, S), "boxes": (C, S, 4), "what": (C, S, 50), "where": (C, S, 4),
              "glimpse": (C, S, 20, 20), "offsets": (S + 1,), "obj_image": (C * S,), "obj_step": (C * S,), "obj_box": (C * S, 4),
              "obj_score": (C * S,), "obj_where": (C * S, 4), "obj_what": (C * S, 50), "reconstruction": (S, 100, 120), "rec": (S,),
              "owner": (S, 100, 120), "area": (C, S), "kept_cand": (C, S), "cand_state": (S, 12 * T), "dup_of": (S, 12 * T),
              "merge_counts": (S, 6), "windows": (S * 12, 50, 50), "window_num_objects": (S, 12), "window_count_prob": (S, 12)}
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes
    assert out["owner"].dtype == torch.int8 and out["cand_state"].dtype == torch.int8 and out["kept_cand"].dtype == torch.int32
    assert torch.isfinite(out["reconstruction"]).all() and torch.isfinite(out["rec"]).all()
    assert (out["merge_counts"].sum(1) == 12 * T).all()
    tp = air.tiled_parser(2, (100, 120))
    assert tp is air.tiled_parser(2, (100, 120)) and tp._graph is not None
    assert torch.equal(tp.engine.flat_params, air._engine.flat_params) and int(tp.engine.step_dev.item()) == 2
    first = {k: v.clone() for k, v in out.items()}
    again = air.parse_tiled(scenes)
    assert all(torch.equal(first[k], again[k]) for k in ("num_objects", "kept_cand", "reconstruction", "owner", "cand_state"))
    ts(); ts_twin()
    air._engine.synchronize(); twin._engine.synchronize()
    assert torch.equal(air._engine.flat_params, twin._engine.flat_params)
    assert torch.equal(air._engine.rng_state, twin._engine.rng_state)
    # a refined, pruned stack is one more cached parser; a third one drops the least recently used
    pruned = air.parse_tiled(scenes, prune="present")
    assert (pruned["num_objects"] <= 32).all() and len(air._tiled_parsers) == 2
    # scoring on annotated scenes
    yy, xx = np.mgrid[0:28, 0:28]
    templates = np.stack([(255 * np.clip(r - np.hypot(yy - 14, xx - 14), 0, 1)).astype(np.uint8) for r in (6, 8, 10, 12)])
    d = create_multi_mnist(templates, canvas_size=(100, 120), n_objects=(0, 4), n_samples=2, return_annotations=True, seed=1)
    annotated = torch.from_numpy(d["imgs"].astype(np.float32) / 255).cuda()
    scores, scorer = air.score_parse_tiled(annotated, d["instances"], d["boxes"], accumulate=False, stride=(50, 50))
    assert len(air._tiled_parsers) == 2                            # the least recently used stack was dropped
    assert scorer.parser is air.tiled_parser(2, (100, 120), (50, 50)) and tuple(scores["box_iou"].shape) == (2, 18, 4)
    summary = scorer.summary()
    assert summary["images"] == 2 and summary["objects_gt"] == int((d["boxes"][..., 2] > 0).sum()) and 0.0 <= summary["count_acc"] <= 1.0
    assert air.obs is obs_before


# ---- 7. scorer ------------------------------------------------------------------------------------------------------------------------
def test_scorer_binds_to_the_tiled_parser(gpu_device):
    """a planted parse scored against itself as ground truth: AP = 1, ARI = 1, count error 0"""
    from attend_infer_repeat_amd.score import ParseScorer
    S = 2
    ocfg, tp, ps, scene = make_tiled("rect_t5", "scene", S)
    img, T = tuple(ocfg.img_size), ocfg.max_steps
    tp.stage(scenes_for(ocfg, scene, S, seed=3).cuda())
    tp.run_segments("gather")
    tp.run_provider()
    tp.synchronize()
    eng = ps.engine
    oy, ox = tile.window_origins(scene, img)
    plant = {(0, 0): scene_row(12.0, 9.0, 10.0, 9.0, scene), (0, 8): scene_row(58.0, 44.0, 12.0, 10.0, scene),
             (1, 4): scene_row(36.0, 28.0, 9.0, 9.0, scene)}
    where, n = eng.where.cpu().numpy().copy(), np.zeros(ps.R, np.int32)
    glimpse = torch.zeros_like(eng.gd.out[-1])
    for (s, v), row in plant.items():
        where[0, s * 9 + v] = unlift(row, scene, img, (oy[v // 3], ox[v % 3])).astype(np.float32)
        n[s * 9 + v] = 1
        glimpse.view(T, ps.R, -1)[0, s * 9 + v] = 1.0               # a bright patch the mask threshold passes
    eng.where.copy_(dev_t(where))
    eng.gd.out[-1].copy_(glimpse)
    ps.num_objects.copy_(dev_t(n))
    ps.score.copy_(torch.linspace(0.9, 0.1, T * ps.R).view(T, ps.R).cuda())
    torch.cuda.synchronize()
    tp.run_segments("merge", "objects", "relabel", "render", "rec_sum")
    tp.synchronize()
    out = tp.result()
    assert out["num_objects"].tolist() == [2, 1] and (out["area"][:2, 0] > 0).all() and out["area"][0, 1] > 0
    scorer = ParseScorer(tp, 3)
    assert (scorer.T, scorer.R) == (tp.T, S)
    gt_boxes = torch.zeros(S, 3, 4).cuda()
    gt_boxes[0, :2], gt_boxes[1, :1] = out["boxes"][:2, 0], out["boxes"][:1, 1]
    scorer.score(out["owner"].clone(), gt_boxes, accumulate=False)
    summary = scorer.summary()
    assert summary["count_acc"] == 1.0 and abs(summary["fg_ari"] - 1.0) < 1e-12
    ap = [v for k, v in summary.items() if k.startswith("ap")]
    assert ap and all(abs(v - 1.0) < 1e-12 for v in ap)


# ---- 8. surface -------------------------------------------------------------------------------------------------------------------------
def test_make_tiled_parse_fig(gpu_device, tmp_path):
    pytest.importorskip("matplotlib")
    from attend_infer_repeat_amd.data import procedural_multi_mnist
    from attend_infer_repeat_amd.evaluation import make_tiled_parse_fig
    air, ts, x, y = _mnist_air(8)
    raw = procedural_multi_mnist(2, (100, 120), (0, 4), seed=5, n_templates=32)
    fig = make_tiled_parse_fig(air, torch.from_numpy(raw["imgs"].astype(np.float32) / 255).cuda(), str(tmp_path), 7, n_samples=2)
    assert fig is not None and os.path.getsize(os.path.join(tmp_path, "tiled_parse_fig_7.png")) > 0


def test_training_script_parse_tiled_option(gpu_device, tmp_path, capsys):
    from attend_infer_repeat_amd.scripts import multi_mnist
    air = multi_mnist.main(["--iters", "3", "--log-every", "3", "--save-every", "1000", "--synthetic-samples", "256",
                            "--eval-batches", "1", "--summary-every", "0", "--results-dir", str(tmp_path), "--parse-tiled", "100x120:25",
                            "--parse-tiled-objects", "4"])
    air._engine.synchronize()
    printed = capsys.readouterr().out
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "multi_mnist", "log.jsonl"))]
    rec = [l for l in lines if l["data"] == "test_parse_tiled_score"]
    assert [l["step"] for l in rec] == [0, 3] and printed.count(" parse tiled score ") == 2
    for l in rec:
        assert l["scene_size"] == [100, 120] and l["stride"] == [25, 25] and l["images"] == 16
        assert 0.0 <= l["count_acc"] <= 1.0 and "map" in l and "fg_ari" in l
        states = [l["merge_" + k] for k in tile.STATES[1:]]
        assert all(v >= 0 for v in states) and sum(states) <= 16 * 12 * 3 and l["merge_kept"] == l["objects_pred"]
