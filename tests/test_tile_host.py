"""Host-side tests of tiled scene parsing (attend_infer_repeat_amd/tile.py): the window grid, the argument checks, the lift -- the
identity at scene == canvas and, with prune._st_write in float64, a window's rendering against the scene-frame rendering of the lifted
row -- `reference_merge` on hand-built scenes, and the new entries in the header and the binding.  No GPU."""
import dataclasses
import os
import re

import numpy as np
import pytest

from attend_infer_repeat_amd import prune, tile
from attend_infer_repeat_amd.engine_config import EngineConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "air_hip.h")


# ---- helpers shared with test_tile.py ---------------------------------------------------------------------------------------------
def unlift(scene_row, scene, img, origin):
    """the window-frame row [sx, tx, sy, ty] (float64) whose lift at `origin` = (oy, ox) is `scene_row`"""
    (Hs, Ws), (H, W), (oy, ox) = scene, img, origin
    ax, ay = (Ws - 1) / (W - 1), (Hs - 1) / (H - 1)
    bx, by = (ax - 1.0) - (2.0 * ox) / (W - 1), (ay - 1.0) - (2.0 * oy) / (H - 1)
    sx, tx, sy, ty = [float(v) for v in scene_row]
    return np.array([sx * ax, tx * ax + bx, sy * ay, ty * ay + by])


def scene_row(cx, cy, bw, bh, scene):
    """the scene-frame row of an object with box centre (cx, cy) and box size (bw, bh), in scene pixels"""
    Hs, Ws = scene
    return np.array([bw / Ws, 2.0 * cx / Ws - 1.0, bh / Hs, 2.0 * cy / Hs - 1.0])


def build_rows(sightings, scene, img, stride, T, S=1, A=3, G=4, seed=0):
    """provider rows from a list of sightings (s, v, cx, cy, bw, bh, score): window v of scene s reports an object with that scene-frame
    box (consecutive steps per window, in list order).  Returns what [T, R, A], where [T, R, 4], glimpse [T, R, G], score [T, R] fp32,
    num_objects [R] int32 and the candidate id of every sighting."""
    oy, ox = tile.window_origins(scene, img, stride)
    Nw = len(oy) * len(ox)
    R = S * Nw
    rng = np.random.default_rng(seed)
    what, glimpse = rng.normal(size=(T, R, A)).astype(np.float32), rng.normal(size=(T, R, G)).astype(np.float32)
    where = np.tile(np.array([0.5, 0.0, 0.5, 0.0], np.float32), (T, R, 1))
    score, n, cands = rng.uniform(size=(T, R)).astype(np.float32), np.zeros(R, np.int32), []
    for (s, v, cx, cy, bw, bh, sc) in sightings:
        r, t = s * Nw + v, int(n[s * Nw + v])
        assert t < T
        where[t, r] = unlift(scene_row(cx, cy, bw, bh, scene), scene, img, (oy[v // len(ox)], ox[v % len(ox)])).astype(np.float32)
        score[t, r] = sc
        n[r] += 1
        cands.append(v * T + t)
    return what, where, glimpse, score, n, cands


def merge_margins(where, score, num_objects, scene, img, stride, iou_merge=0.5):
    """how far the decisions of reference_merge are from flipping, per scene: (centre [S]: the smallest distance in pixels of a finite
    present candidate's box centre from a boundary of its window's cell;  iou [S]: the smallest |IoU - iou_merge| over the pairs of
    owned candidates of different windows;  ties [S]: pairs of owned candidates with equal scores)"""
    where, score = np.asarray(where, np.float32), np.asarray(score, np.float32)
    T, R = score.shape
    (Hs, Ws), (H, W) = scene, img
    oy, ox = tile.window_origins(scene, img, stride)
    nx, Nw = len(ox), len(oy) * len(ox)
    S = R // Nw
    (ylo, yhi), (xlo, xhi) = tile.cell_bounds(oy, H), tile.cell_bounds(ox, W)
    centre, iou, ties = np.full(S, np.inf), np.full(S, np.inf), np.zeros(S, np.int64)
    for s in range(S):
        owned = []
        for c in range(Nw * T):
            v, t = divmod(c, T)
            i, j = divmod(v, nx)
            r = s * Nw + v
            if t >= num_objects[r]:
                continue
            with np.errstate(all="ignore"):
                row = tile.reference_lift(where[t, r], scene, img, (oy[i], ox[j])).astype(np.float32)
            if not (np.isfinite(row).all() and np.isfinite(score[t, r])):
                continue
            cy, cx = tile.scene_centres(row, scene)
            d = min(abs(cx - b) for b in (xlo[j], xhi[j])), min(abs(cy - b) for b in (ylo[i], yhi[i]))
            centre[s] = min(centre[s], *d)
            if xlo[j] <= cx < xhi[j] and ylo[i] <= cy < yhi[i]:
                owned.append((c, tile.scene_boxes(row, scene), score[t, r]))
        for a in range(len(owned)):
            for b in range(a + 1, len(owned)):
                ties[s] += owned[a][2] == owned[b][2]
                if owned[a][0] // T != owned[b][0] // T:
                    iou[s] = min(iou[s], abs(tile.box_iou(owned[a][1], owned[b][1]) - iou_merge))
    return centre, iou, ties


# ---- 1. window_origins ------------------------------------------------------------------------------------------------------------
def test_window_origins_clamp_the_last_window():
    oy, ox = tile.window_origins((7, 9), (5, 6), (2, 3))
    assert oy.tolist() == [0, 2] and ox.tolist() == [0, 3]
    oy, ox = tile.window_origins((100, 120), (50, 50))
    assert oy.tolist() == [0, 25, 50] and ox.tolist() == [0, 25, 50, 70]            # 75 clamped to 120 - 50
    oy, ox = tile.window_origins((50, 50), (50, 50), (7, 50))
    assert oy.tolist() == [0] and ox.tolist() == [0]


def test_windows_cover_every_pixel():
    rng = np.random.default_rng(0)
    for _ in range(200):
        H, W = rng.integers(2, 12, 2)
        Hs, Ws = H + rng.integers(0, 30), W + rng.integers(0, 30)
        sy, sx = rng.integers(1, H + 1), rng.integers(1, W + 1)
        oy, ox = tile.window_origins((Hs, Ws), (H, W), (sy, sx))
        assert oy[0] == 0 and ox[0] == 0 and oy[-1] == Hs - H and ox[-1] == Ws - W
        assert (np.diff(oy) > 0).all() and (np.diff(ox) > 0).all() and (np.diff(oy) <= sy).all() and (np.diff(ox) <= sx).all()
        seen = np.zeros((Hs, Ws), bool)
        for y in oy:
            for x in ox:
                seen[y:y + H, x:x + W] = True
        assert seen.all()
        ref = tile.reference_gather(np.arange(Hs * Ws, dtype=np.float32).reshape(1, Hs, Ws), (H, W), (sy, sx))
        assert ref.shape == (len(oy) * len(ox), H * W) and ref[-1, -1] == Hs * Ws - 1 and ref[0, 0] == 0


# ---- 2. check_arguments -----------------------------------------------------------------------------------------------------------
def test_check_arguments_accepts_and_gives_the_default_stride():
    cfg = EngineConfig(max_steps=3)
    H, W = cfg.img_size
    assert tile.check_arguments(cfg, (2 * H, 2 * W + 20)) == ((2 * H, 2 * W + 20), (H // 2, W // 2), (3, 4))
    assert tile.check_arguments(cfg, (H, W))[2] == (1, 1)
    tile.check_arguments(dataclasses.replace(cfg, max_steps=32), (H, 2 * W), (H, W))       # 2 windows * 32 steps


@pytest.mark.parametrize("change,scene,stride,iou,n,match", [
    (dict(), (49, 50), None, 0.5, 1, "smaller than"), (dict(), (50, 20), None, 0.5, 1, "smaller than"),
    (dict(), (100, 100), (0, 25), 0.5, 1, "stride"), (dict(), (100, 100), (25, 51), 0.5, 1, "stride"),
    (dict(), (100, 100), (25, -1), 0.5, 1, "stride"),
    (dict(), (200, 200), (10, 10), 0.5, 1, "candidates"),                       # 16 * 16 windows * 3
    (dict(max_steps=33), (50, 50), None, 0.5, 1, "max_steps"), (dict(max_steps=0), (50, 50), None, 0.5, 1, "max_steps"),
    (dict(img_size=(1, 50)), (50, 50), (1, 25), 0.5, 1, "2 x 2"), (dict(img_size=(50, 1)), (50, 50), (25, 1), 0.5, 1, "2 x 2"),
    (dict(), (100, 100), None, 0.5, 2 ** 31 // 9 + 1, "int32"),
    (dict(), (100, 100), None, float("nan"), 1, "iou_merge"), (dict(), (100, 100), None, 1.5, 1, "iou_merge"),
    (dict(), (100, 100), None, -0.1, 1, "iou_merge")])
def test_check_arguments_refuses(change, scene, stride, iou, n, match):
    with pytest.raises(ValueError, match=match):
        tile.check_arguments(dataclasses.replace(EngineConfig(max_steps=3), **change), scene, stride, iou, n)


# ---- 3. reference_lift ------------------------------------------------------------------------------------------------------------
def test_lift_is_the_identity_at_scene_equal_canvas():
    rng = np.random.default_rng(1)
    w = rng.normal(size=(64, 4)).astype(np.float32)
    w[0] = [0.0, -0.0, np.inf, -np.inf]
    w[1] = np.float32(1e-42)                                       # denormal
    out = tile.reference_lift(w, (50, 37), (50, 37), (0, 0)).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("origin", [(0, 0), (25, 50), (50, 70)])        # a corner, inside, both clamped edges of 100 x 120
def test_lifted_row_renders_the_window_inside_the_scene(origin):
    scene, img, (h, w) = (100, 120), (50, 50), (7, 6)
    rng = np.random.default_rng(sum(origin))
    glimpse = rng.normal(size=(4, h, w))
    where = np.array([[0.4, 0.1, 0.5, -0.2], [0.3, 0.85, 0.6, 0.0], [-0.5, -0.9, 0.35, 0.95], [1.3, 0.0, 1.2, 0.1]])
    lifted = tile.reference_lift(where, scene, img, origin)
    in_window = prune._st_write(glimpse, where, img)
    in_scene = prune._st_write(glimpse, lifted, scene)
    oy, ox = origin
    assert np.abs(in_window).max() > 0.1
    worst = np.abs(in_scene[:, oy:oy + img[0], ox:ox + img[1]] - in_window).max()
    assert worst <= 1e-12, worst
    # the lifted row also renders what the window cut off: rows 1 and 2 reach over the window's edge
    outside = in_scene.copy()
    outside[:, oy:oy + img[0], ox:ox + img[1]] = 0
    if origin == (25, 50):
        assert np.abs(outside[1]).max() > 0 and np.abs(outside[3]).max() > 0


def test_scene_box_is_not_window_box_plus_origin():
    """attention_box scales by W, the transformer grid by W - 1: the authoritative scene box is off "window box + origin" by
    ox / (Ws - 1) - l (Ws - W) / (W (Ws - 1)) pixels, below 0.6 px at 50 -> 120"""
    from attend_infer_repeat_amd.evaluation import attention_box
    rng = np.random.default_rng(2)
    (Hs, Ws), (H, W) = (100, 120), (50, 50)
    worst = 0.0
    for _ in range(200):
        ox, oy = rng.integers(0, Ws - W + 1), rng.integers(0, Hs - H + 1)
        bw, bh = rng.uniform(5, 25, 2)
        l, t = rng.uniform(0, W - bw), rng.uniform(0, H - bh)
        row = np.array([bw / W, 2 * (l + bw / 2) / W - 1, bh / H, 2 * (t + bh / 2) / H - 1])
        assert np.allclose(attention_box(row, W, H), (l, t, bw, bh))
        left, top, width, height = attention_box(tile.reference_lift(row, (Hs, Ws), (H, W), (oy, ox)), Ws, Hs)
        assert abs((left - (ox + l)) - (ox / (Ws - 1) - l * (Ws - W) / (W * (Ws - 1)))) < 1e-9
        assert abs(width - bw * Ws * (W - 1) / (W * (Ws - 1))) < 1e-9
        worst = max(worst, abs(left - (ox + l)), abs(top - (oy + t)))
    assert 0.3 < worst < 0.6, worst


def test_unlift_inverts_the_lift():
    row = scene_row(61.0, 40.0, 18.0, 22.0, (100, 120))
    back = tile.reference_lift(unlift(row, (100, 120), (50, 50), (25, 50)), (100, 120), (50, 50), (25, 50))
    assert np.abs(back - row).max() < 1e-15


# ---- 4. reference_merge on hand-built scenes ------------------------------------------------------------------------------------------
SCENE, IMG, STRIDE = (10, 20), (10, 10), (5, 5)                    # one row of three windows at ox = 0, 5, 10: cells split at 7.5, 12.5


def merge(sightings, T=2, scene=SCENE, img=IMG, stride=STRIDE, **kw):
    what, where, glimpse, score, n, cands = build_rows(sightings, scene, img, stride, T, **kw)
    return tile.reference_merge(what, where, glimpse, score, n, scene, img, stride, kw.get("iou_merge", 0.5)), cands, \
        (what, where, glimpse, score, n)


def test_merge_one_object_seen_by_two_windows_is_kept_once():
    # window 0 puts the centre at 7.4 (its own cell), window 1 at 7.6 (its own cell): IoU 3.8 / 4.2; and window 0 also reports a
    # truncated sighting centred at 9, which is window 1's cell
    out, (c0, c1, c2), rows = merge([(0, 0, 7.4, 5.0, 4.0, 4.0, 0.9), (0, 1, 7.6, 5.0, 4.0, 4.0, 0.8), (0, 0, 9.0, 2.0, 2.0, 2.0, 0.99)])
    assert (c0, c1, c2) == (0, 2, 1)
    assert out["cand_state"][0].tolist() == [tile.KEPT, tile.NOT_OWNED, tile.DUPLICATE, tile.ABSENT, tile.ABSENT, tile.ABSENT]
    assert out["dup_of"][0].tolist() == [-1, -1, 0, -1, -1, -1]
    assert out["num_objects"].tolist() == [1] and out["kept_cand"][:, 0].tolist() == [0, -1, -1, -1, -1, -1]
    assert out["merge_counts"][0].tolist() == [3, 1, 1, 1, 0, 0]
    what, where, glimpse, score, n = rows
    assert np.array_equal(out["what"][0, 0], what[0, 0]) and np.array_equal(out["glimpse"][0, 0], glimpse[0, 0])
    assert out["score_src"][0, 0] == np.float32(0.9)
    assert np.allclose(out["where"][0, 0], scene_row(7.4, 5.0, 4.0, 4.0, SCENE), atol=1e-6)
    assert (out["what"][1:] == 0).all()
    # the better score wins whichever window it is
    out, _, _ = merge([(0, 0, 7.4, 5.0, 4.0, 4.0, 0.7), (0, 1, 7.6, 5.0, 4.0, 4.0, 0.8)])
    assert out["cand_state"][0].tolist()[:3] == [tile.DUPLICATE, tile.ABSENT, tile.KEPT] and out["dup_of"][0, 0] == 2
    # below the threshold both stay: IoU 2 / 6
    out, _, _ = merge([(0, 0, 6.5, 5.0, 4.0, 4.0, 0.7), (0, 1, 8.5, 5.0, 4.0, 4.0, 0.8)])
    assert out["num_objects"].tolist() == [2]


def test_merge_never_suppresses_inside_one_window():
    out, cands, _ = merge([(0, 1, 9.0, 5.0, 4.0, 4.0, 0.9), (0, 1, 9.2, 5.0, 4.0, 4.0, 0.8)])
    assert cands == [2, 3] and out["num_objects"].tolist() == [2] and out["kept_cand"][:2, 0].tolist() == [2, 3]
    assert (out["dup_of"] == -1).all()


def test_merge_centre_on_the_boundary_belongs_to_the_higher_window():
    # canvas 5 x 5, scene 5 x 9, stride 4: ox = 0, 4, beta_0 = 4.5 = Ws / 2: tx' = 0, which both windows' rows lift to exactly
    scene, img, stride = (5, 9), (5, 5), (5, 4)
    what, where, glimpse, score, n, cands = build_rows([(0, 0, 4.5, 2.5, 2.0, 2.0, 0.9), (0, 1, 4.5, 2.5, 2.0, 2.0, 0.1)], scene, img,
                                                       stride, 1)
    assert where[0, 0, 1] == 1.0 and where[0, 1, 1] == -1.0
    out = tile.reference_merge(what, where, glimpse, score, n, scene, img, stride)
    assert out["where_lifted"][0, :, 1].tolist() == [0.0, 0.0]
    assert out["cand_state"][0].tolist() == [tile.NOT_OWNED, tile.KEPT] and out["kept_cand"][0, 0] == 1


def test_merge_equal_scores_the_lower_candidate_wins():
    out, cands, _ = merge([(0, 1, 7.6, 5.0, 4.0, 4.0, 0.5), (0, 0, 7.4, 5.0, 4.0, 4.0, 0.5)])
    assert cands == [2, 0]
    assert out["cand_state"][0, [0, 2]].tolist() == [tile.KEPT, tile.DUPLICATE] and out["dup_of"][0, 2] == 0


def test_merge_nonfinite_rows():
    for k, bad in ((0, np.nan), (1, np.inf), (3, -np.inf), (None, np.nan)):
        what, where, glimpse, score, n, _ = build_rows([(0, 0, 3.0, 5.0, 4.0, 4.0, 0.9), (0, 1, 9.0, 5.0, 2.0, 2.0, 0.8)], SCENE, IMG,
                                                       STRIDE, 2)
        if k is None:
            score[0, 0] = bad
        else:
            where[0, 0, k] = bad
        out = tile.reference_merge(what, where, glimpse, score, n, SCENE, IMG, STRIDE)
        assert out["cand_state"][0].tolist() == [tile.NONFINITE, 0, tile.KEPT, 0, 0, 0]
        assert out["num_objects"].tolist() == [1] and out["merge_counts"][0].tolist() == [4, 1, 0, 0, 0, 1]


def overflow_case():
    """ten disjoint windows of four objects each: 40 owned candidates that overlap nothing"""
    scene, img, stride, T = (10, 100), (10, 10), (10, 10), 4
    rng = np.random.default_rng(5)
    scores = rng.permutation(40).astype(np.float64) / 64 + 0.125
    sightings = [(0, v, 10 * v + 2.0 + 2 * t, 5.0, 1.0, 1.0, scores[v * T + t]) for v in range(10) for t in range(T)]
    return sightings, scene, img, stride, T, scores


def test_merge_overflow_drops_the_lowest_scores():
    sightings, scene, img, stride, T, scores = overflow_case()
    out, cands, _ = merge(sightings, T, scene, img, stride)
    assert cands == list(range(40))
    state = out["cand_state"][0]
    assert (state == tile.KEPT).sum() == 32 and (state == tile.OVERFLOW).sum() == 8 and out["num_objects"].tolist() == [32]
    assert sorted(np.flatnonzero(state == tile.OVERFLOW).tolist()) == sorted(np.argsort(scores)[:8].tolist())
    assert out["kept_cand"][:, 0].tolist() == np.flatnonzero(state == tile.KEPT).tolist()
    assert out["merge_counts"][0].tolist() == [0, 32, 0, 0, 8, 0]


def test_merge_all_absent():
    what, where, glimpse, score, n, _ = build_rows([], SCENE, IMG, STRIDE, 2, S=3)
    out = tile.reference_merge(what, where, glimpse, score, n, SCENE, IMG, STRIDE)
    assert out["num_objects"].tolist() == [0, 0, 0] and (out["cand_state"] == 0).all() and (out["kept_cand"] == -1).all()
    assert out["merge_counts"].tolist() == [[6, 0, 0, 0, 0, 0]] * 3


def test_merge_one_window_is_the_identity():
    rng = np.random.default_rng(3)
    T, R, A, G = 3, 5, 4, 6
    what, where, glimpse = (rng.normal(size=(T, R, k)).astype(np.float32) for k in (A, 4, G))
    score, n = rng.uniform(size=(T, R)).astype(np.float32), np.array([0, 1, 2, 3, 3], np.int32)
    where[:, 4] = where[:, 3]                                      # the same boxes twice in one window: both stay
    out = tile.reference_merge(what, where, glimpse, score, n, (8, 9), (8, 9), None)
    assert out["num_objects"].tolist() == n.tolist()
    for r in range(R):
        for k, src in (("what", what), ("where", where), ("glimpse", glimpse)):
            assert np.array_equal(out[k][:n[r], r].view(np.uint32), src[:n[r], r].view(np.uint32))
        assert out["kept_cand"][:, r].tolist() == list(range(n[r])) + [-1] * (T - n[r])


# ---- 5. the entries -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_on_the_engine_side_and_bound():
    from attend_infer_repeat_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("air_tile_gather", 10), ("air_tile_merge", 26), ("air_tile_relabel", 10)):
        m = re.search(r"AIR_ENGINE_API\s+int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert "tile_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "tile_kernels.hip"))
    assert _lib.ABI_VERSION == 10 and _lib.ENGINE_ABI_VERSION == 5


def test_argument_checks_need_no_device():
    """NULL / bad-shape / misaligned arguments return AIR_E_* before any launch"""
    import ctypes
    from attend_infer_repeat_amd import _lib, build
    build.build()
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                                  # any non-NULL, 16-byte aligned host address: never dereferenced
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, p4 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    gather = lambda S=1, Hs=8, Ws=8, H=4, W=4, sy=2, sx=2, a=p, b=p: lib.air_tile_gather(a, S, Hs, Ws, H, W, sy, sx, b, None)
    assert gather(a=None) == -1 and gather(b=None) == -1
    for kw in (dict(Hs=3), dict(Ws=3), dict(sy=0), dict(sy=5), dict(sx=0), dict(sx=5), dict(S=0), dict(H=1, Hs=1, sy=1), dict(W=1, sx=1),
               dict(S=2 ** 31 - 1), dict(Hs=2 ** 16, Ws=2 ** 15)):
        assert gather(**kw) == -2, kw
    assert gather(a=ctypes.c_void_p(base + 2)) == -3

    def merge(T=3, S=1, Hs=8, Ws=8, H=4, W=4, sy=2, sx=2, where=p, where_out=p, what=p, cand_state=p):
        return lib.air_tile_merge(what, where, p, p, p, T, S, 4, 4, Hs, Ws, H, W, sy, sx, 0.5, p, where_out, p, p, p, p, cand_state, p, p,
                                  None)
    assert merge(what=None) == -1 and merge(cand_state=None) == -1
    for kw in (dict(T=0), dict(T=33), dict(Hs=3), dict(sy=5), dict(sx=0), dict(H=1, Hs=1, sy=1), dict(S=0),
               dict(Hs=64, Ws=64, sy=1, sx=1),                     # 61 * 61 windows
               dict(T=32)):                                        # 9 windows * 32
        assert merge(**kw) == -2, kw
    assert merge(where=p4) == -3 and merge(where_out=p4) == -3 and merge(what=ctypes.c_void_p(base + 2)) == -3
    assert lib.air_tile_relabel(None, p, p, p, 3, 1, p, p, p, None) == -1
    for C in (0, 33):
        assert lib.air_tile_relabel(p, p, p, p, C, 1, p, p, p, None) == -2
    assert lib.air_tile_relabel(p, p, p, p, 3, 0, p, p, p, None) == -2
