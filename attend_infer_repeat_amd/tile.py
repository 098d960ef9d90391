"""Parsing scenes larger than the model's canvas on the device: overlapping windows, parsed by a bound provider, merged per scene.

The spatial transformer works in normalised coordinates, so a window's object is a scene's object once its `where` row is re-expressed
in the scene's frame (the lift below); what remains is bookkeeping: which window owns an object, and which sightings of two windows are
the same object.

Sizes.  Canvas H x W (both > 1), scene Hs x Ws (Hs >= H, Ws >= W), stride (sy, sx) with 1 <= sy <= H, 1 <= sx <= W, default
(H // 2, W // 2).  ny = 1 + ceil((Hs - H) / sy) windows along y at oy_i = min(i sy, Hs - H) -- the last one is clamped to the edge,
nothing is padded -- nx / ox_j alike; Nw = ny nx, window v = i nx + j, window row r = s Nw + v.  Candidate c = v T + t,
Nc = Nw T <= 256 per scene; the merged scene has C = min(Nc, 32) slots.

Lift of where = [sx, tx, sy, ty] (float64 on the fp32 row, this operation order, rounded once to fp32):
    ax = (Ws - 1) / (W - 1),  bx = (ax - 1) - (2 ox) / (W - 1),  sx' = sx / ax,  tx' = (tx - bx) / ax;   y alike with Hs, H, oy.
The scene box of a candidate is evaluation.attention_box(where', Ws, Hs) in fp32, what air_parse_objects forms from the lifted row.

State of a candidate, decided in this order: 0 absent (t >= the window's count), 5 non-finite (a lifted value or the score), 2 not
owned (the box centre cx = Ws (1 + tx') / 2, cy = Hs (1 + ty') / 2 lies outside the half-open cell [beta_{j-1}, beta_j) of its own
window, beta_j = (ox_{j+1} + ox_j + W) / 2 the middle of the overlap), 3 duplicate (walking the owned candidates by score descending,
the lower c first between equal scores: a candidate kept before it, of ANOTHER window, has float64 box IoU > iou_merge with it,
strictly; dup_of = the first such one in walk order), 4 overflow (C are kept already; it suppresses nothing), 1 kept.  The kept
candidates fill slots 0 .. n-1 in ascending c.  Candidates of one window never suppress each other, so one window is the identity.

`TiledSceneParser` owns no engine: it binds to a parse.SceneParser, refine.ParseRefiner, prune.ParsePruner or propose.ParseProposer
at R = S Nw rows, cuts the scenes into that provider's rows (air_tile_gather), runs the provider's own `parse()` and then, on the same
engine stream, its own launch list of libair_hip.so entries (include/air_hip.h), ONE hipGraph after `capture()`:

  air_tile_merge     lift, ownership, suppression, compaction (above);
  air_parse_objects  (given counts, no presence_prob) on the compacted rows at T := C, R := S, image Hs x Ws: boxes and the table;
  air_tile_relabel   score / obj_score = the windows' scores, obj_step = the candidate id (obj_step // T is the window) --
                     air_prune_relabel's rule, which that entry applies to at most 6 rows;
  air_parse_render, air_sum_leading   reconstruction, rec, owner, area of the scene.

Known waste: the provider copies the windows into its engine's `obs` (one device-to-device copy of the gathered bytes).
`reference_gather`, `reference_lift` and `reference_merge` restate the definitions in numpy float64.
"""
import math
from collections import OrderedDict
from typing import Dict

from .stage import BoundStage, ReadOut, compacted_rows

MAX_SLOTS = 32                     # PARSE_MAXT / SCORE_MAXT; the owner map is int8
MAX_CANDIDATES = 256               # air_tile_merge: one thread per candidate
ABSENT, KEPT, NOT_OWNED, DUPLICATE, OVERFLOW, NONFINITE = range(6)
STATES = ("absent", "kept", "not_owned", "duplicate", "overflow", "nonfinite")
INT32_MAX = 2 ** 31 - 1


def _pair(v, name):
    try:
        a, b = v
    except TypeError:
        a = b = v
    if int(a) != a or int(b) != b:
        raise ValueError("%s must be integers, got %r" % (name, v))
    return int(a), int(b)


def window_count(scene: int, window: int, stride: int) -> int:
    return 1 + -(-(scene - window) // stride)


def check_geometry(scene_size, img_size, stride=None, max_steps=None, n_scenes: int = 1):
    """the refusals of air_tile_gather and, with `max_steps` given, of air_tile_merge on plain sizes; returns
    ((Hs, Ws), (sy, sx), (ny, nx))"""
    (Hs, Ws), (H, W) = _pair(scene_size, "scene_size"), _pair(img_size, "img_size")
    if H <= 1 or W <= 1:
        raise ValueError("tiling needs a canvas of at least 2 x 2 pixels (the lift divides by H - 1 and W - 1), got %r" % ((H, W),))
    if Hs < H or Ws < W:
        raise ValueError("the scene %r is smaller than the model's canvas %r" % ((Hs, Ws), (H, W)))
    sy, sx = (H // 2, W // 2) if stride is None else _pair(stride, "stride")
    if not (1 <= sy <= H and 1 <= sx <= W):
        raise ValueError("the stride must be within 1..%d x 1..%d so that the windows cover the scene, got %r" % (H, W, (sy, sx)))
    ny, nx = window_count(Hs, H, sy), window_count(Ws, W, sx)
    T = 0 if max_steps is None else int(max_steps)
    if max_steps is not None and not 1 <= T <= MAX_SLOTS:
        raise ValueError("max_steps must be within 1..%d, got %d" % (MAX_SLOTS, T))
    if ny * nx * T > MAX_CANDIDATES:
        raise ValueError("%d x %d windows of %d steps are %d candidates per scene; the merge takes at most %d: use a larger stride"
                         % (ny, nx, T, ny * nx * T, MAX_CANDIDATES))
    if int(n_scenes) < 1 or int(n_scenes) * ny * nx > INT32_MAX or Hs * Ws > INT32_MAX // 2:
        raise ValueError("n_scenes * windows (%d * %d) and the scene's pixels must stay within int32" % (int(n_scenes), ny * nx))
    return (Hs, Ws), (sy, sx), (ny, nx)


def check_arguments(cfg, scene_size, stride=None, iou_merge: float = 0.5, n_scenes: int = 1):
    """Refuse what cannot be tiled (pure host code: importable and callable without a GPU).  Returns ((Hs, Ws), (sy, sx), (ny, nx))."""
    iou = float(iou_merge)
    if not (math.isfinite(iou) and 0.0 <= iou <= 1.0):
        raise ValueError("iou_merge must be a number within [0, 1], got %r" % (iou_merge,))
    return check_geometry(scene_size, cfg.img_size, stride, int(cfg.max_steps), n_scenes)


def window_origins(scene_size, img_size, stride=None):
    """(oy [ny], ox [nx]) int64: the windows' top-left corners, the last one clamped to the edge"""
    import numpy as np
    (Hs, Ws), (sy, sx), (ny, nx) = check_geometry(scene_size, img_size, stride)
    H, W = _pair(img_size, "img_size")
    return np.minimum(np.arange(ny) * sy, Hs - H).astype(np.int64), np.minimum(np.arange(nx) * sx, Ws - W).astype(np.int64)


def reference_gather(scenes, img_size, stride=None):
    """air_tile_gather in numpy: scenes [S, Hs, Ws] -> [S * Nw, H * W], row s * Nw + i * nx + j"""
    import numpy as np
    scenes = np.asarray(scenes)
    S, Hs, Ws = scenes.shape
    H, W = _pair(img_size, "img_size")
    oy, ox = window_origins((Hs, Ws), (H, W), stride)
    out = np.empty((S, len(oy) * len(ox), H * W), scenes.dtype)
    for i, y in enumerate(oy):
        for j, x in enumerate(ox):
            out[:, i * len(ox) + j] = scenes[:, y:y + H, x:x + W].reshape(S, -1)
    return out.reshape(-1, H * W)


def reference_lift(where, scene_size, img_size, origin):
    """the lift in float64, NOT yet rounded: where [..., 4] = [sx, tx, sy, ty] (any float dtype), origin = (oy, ox), each a number or
    an array broadcasting against where[..., 0]"""
    import numpy as np
    w = np.asarray(where, np.float64)
    (Hs, Ws), (H, W) = _pair(scene_size, "scene_size"), _pair(img_size, "img_size")
    if H <= 1 or W <= 1:
        raise ValueError("the lift divides by H - 1 and W - 1: a canvas of %r cannot be lifted" % ((H, W),))
    oy, ox = np.asarray(origin[0], np.float64), np.asarray(origin[1], np.float64)
    out = np.empty(w.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for (sc, sh, scene, window, o) in ((0, 1, Ws, W, ox), (2, 3, Hs, H, oy)):
            a = np.float64(scene - 1) / np.float64(window - 1)
            b = (a - 1.0) - (2.0 * o) / np.float64(window - 1)
            out[..., sc] = w[..., sc] / a
            out[..., sh] = (w[..., sh] - b) / a
    return out


def scene_boxes(where32, scene_size):
    """evaluation.attention_box in fp32, operation by operation as air_parse_objects forms it: [..., 4] = (left, top, width, height)"""
    import numpy as np
    w = np.asarray(where32, np.float32)
    Hf, Wf, one, half = np.float32(scene_size[0]), np.float32(scene_size[1]), np.float32(1), np.float32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([Wf * ((one - w[..., 0]) + w[..., 1]) * half, Hf * ((one - w[..., 2]) + w[..., 3]) * half,
                         Wf * w[..., 0], Hf * w[..., 2]], -1).astype(np.float32)


def scene_centres(where32, scene_size):
    """(cy, cx) in float64 from the lifted fp32 row"""
    import numpy as np
    w = np.asarray(where32, np.float32).astype(np.float64)
    return (scene_size[0] * (1.0 + w[..., 3])) / 2.0, (scene_size[1] * (1.0 + w[..., 1])) / 2.0


def cell_bounds(origins, window: int):
    """(lo [n], hi [n]) float64: window i owns [lo_i, hi_i) along one axis"""
    import numpy as np
    o = np.asarray(origins, np.float64)
    beta = (o[1:] + o[:-1] + window) / 2.0
    return np.concatenate([[-np.inf], beta]), np.concatenate([beta, [np.inf]])


def box_iou(a, b) -> float:
    """air_score_match's float64 box IoU of two fp32 (left, top, width, height) boxes"""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if any(math.isnan(v) for v in a + b):
        return 0.0
    ax0, ax1, ay0, ay1 = min(a[0], a[0] + a[2]), max(a[0], a[0] + a[2]), min(a[1], a[1] + a[3]), max(a[1], a[1] + a[3])
    bx0, bx1, by0, by1 = min(b[0], b[0] + b[2]), max(b[0], b[0] + b[2]), min(b[1], b[1] + b[3]), max(b[1], b[1] + b[3])
    iw, ih = max(0.0, min(ax1, bx1) - max(ax0, bx0)), max(0.0, min(ay1, by1) - max(ay0, by0))
    inter = iw * ih
    union = ((ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0)) - inter
    if not (inter > 0 and union > 0):
        return 0.0
    q = inter / union
    return q if math.isfinite(q) else 0.0


def reference_merge(what, where, glimpse, score, num_objects, scene_size, img_size, stride=None, iou_merge: float = 0.5):
    """air_tile_merge restated in numpy float64.  Arrays as the kernel takes them: what [T, R, A], where [T, R, 4], glimpse [T, R, G],
    score [T, R], num_objects [R], R = S * Nw.  Returns cand_state [S, Nc] int8, dup_of [S, Nc] int32, merge_counts [S, 6] int32,
    num_objects [S] int32, kept_cand [C, S] int32 (-1 beyond the count), where_lifted [S, Nc, 4] float32 (every candidate's lifted
    row), and what [C, S, A], where [C, S, 4], glimpse [C, S, G], score_src [C, S] with zeros in the rows the kernel does not write."""
    import numpy as np
    what, where, glimpse, score = (np.asarray(a, np.float32) for a in (what, where, glimpse, score))
    n_in = np.asarray(num_objects).astype(np.int64)
    T, R, A = what.shape
    G = glimpse.shape[2]
    H, W = _pair(img_size, "img_size")
    (Hs, Ws), (sy, sx), (ny, nx) = check_geometry(scene_size, (H, W), stride, T)
    oy, ox = window_origins((Hs, Ws), (H, W), (sy, sx))
    Nw = ny * nx
    if R % Nw:
        raise ValueError("%d rows are no multiple of %d windows" % (R, Nw))
    S, Nc, C = R // Nw, Nw * T, min(Nw * T, MAX_SLOTS)
    (ylo, yhi), (xlo, xhi) = cell_bounds(oy, H), cell_bounds(ox, W)
    thr = float(iou_merge)
    out = {"cand_state": np.zeros((S, Nc), np.int8), "dup_of": np.full((S, Nc), -1, np.int32),
           "merge_counts": np.zeros((S, 6), np.int32), "num_objects": np.zeros(S, np.int32),
           "kept_cand": np.full((C, S), -1, np.int32), "where_lifted": np.zeros((S, Nc, 4), np.float32),
           "what": np.zeros((C, S, A), np.float32), "where": np.zeros((C, S, 4), np.float32),
           "glimpse": np.zeros((C, S, G), np.float32), "score_src": np.zeros((C, S), np.float32)}
    for s in range(S):
        state = out["cand_state"][s]
        lifted, boxes, owned = np.zeros((Nc, 4), np.float32), np.zeros((Nc, 4), np.float32), []
        for c in range(Nc):
            v, t = divmod(c, T)
            i, j = divmod(v, nx)
            r = s * Nw + v
            if t >= n_in[r]:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                lifted[c] = reference_lift(where[t, r], (Hs, Ws), (H, W), (oy[i], ox[j])).astype(np.float32)
            if not (np.isfinite(lifted[c]).all() and np.isfinite(score[t, r])):
                state[c] = NONFINITE
                continue
            boxes[c] = scene_boxes(lifted[c], (Hs, Ws))
            cy, cx = scene_centres(lifted[c], (Hs, Ws))
            if not (xlo[j] <= cx < xhi[j] and ylo[i] <= cy < yhi[i]):
                state[c] = NOT_OWNED
                continue
            owned.append(c)
        sc = lambda c: score[c % T, s * Nw + c // T]
        kept = []
        for c in sorted(owned, key=lambda c: (-float(sc(c)), c)):
            by = next((k for k in kept if k // T != c // T and box_iou(boxes[k], boxes[c]) > thr), None)
            if by is not None:
                state[c], out["dup_of"][s, c] = DUPLICATE, by
            elif len(kept) == C:
                state[c] = OVERFLOW
            else:
                state[c] = KEPT
                kept.append(c)
        out["where_lifted"][s] = lifted
        out["num_objects"][s] = len(kept)
        out["merge_counts"][s] = np.bincount(state, minlength=6)
        for slot, c in enumerate(sorted(kept)):
            t, r = c % T, s * Nw + c // T
            out["kept_cand"][slot, s] = c
            out["what"][slot, s], out["glimpse"][slot, s], out["score_src"][slot, s] = what[t, r], glimpse[t, r], score[t, r]
            out["where"][slot, s] = lifted[c]
    return out


def _provider_rows(provider):
    """the device buffers of the provider's `parse()` that the merge reads (its rows()), or the refusal"""
    return TiledSceneParser.bind(provider)


class TiledSceneParser(BoundStage):
    KIND = "tiled"
    ACCEPTS = ("scene", "refiner", "subset")
    REFUSALS = {"particle": "a ParticleParser is out of scope for tiling (its rows are particles of an image, not images): bind a "
                            "SceneParser, ParseRefiner, ParsePruner or ParseProposer"}
    KEY_FIELDS = ("output_multiplier", "output_std")

    def __init__(self, provider, scene_size, stride=None, iou_merge: float = 0.5):
        rows = self.bind(provider)
        cfg = provider.engine.cfg
        (Hs, Ws), (sy, sx), (ny, nx) = check_arguments(cfg, scene_size, stride, iou_merge)
        Nw = ny * nx
        if provider.R % Nw:
            raise ValueError("the provider's %d rows are no multiple of the %d windows of a %d x %d scene at stride %r"
                             % (provider.R, Nw, Hs, Ws, (sy, sx)))
        check_arguments(cfg, scene_size, stride, iou_merge, provider.R // Nw)
        import torch
        from . import hip as H
        self.provider, self.engine = provider, provider.engine
        self._bound = provider
        self.scene_size, self.stride, self.grid, self.iou_merge = (Hs, Ws), (sy, sx), (ny, nx), float(iou_merge)
        self.n_windows, self.window_T = Nw, int(provider.T)
        self.T, self.R = min(Nw * self.window_T, MAX_SLOTS), provider.R // Nw
        self.mask_threshold = provider.mask_threshold
        self._rows = rows
        eng, dev = self.engine, self.engine.device
        C, S, A, Nc = self.T, self.R, int(cfg.n_appearance), Nw * self.window_T
        (Hi, Wi), hw = cfg.img_size, cfg.n_crop
        self.n_bands = int(H.lib().air_canvas_unroll_bands(S, Hs))
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.scenes, self.windows = z((S, Hs, Ws)), z((S * Nw, Hi * Wi))
            self.what, self.where, self.glimpse, self.score_src = z((C, S, A)), z((C, S, 4)), z((C, S, hw)), z((C, S))
            self.kept_cand = torch.full((C, S), -1, dtype=torch.int32, device=dev)
            self.num_objects_in = z((S,), torch.int32)
            self.cand_state, self.dup_of = z((S, Nc), torch.int8), torch.full((S, Nc), -1, dtype=torch.int32, device=dev)
            self.merge_counts = z((S, 6), torch.int32)
        # the read-out of the scene (what the parsers keep)
        self._ro = ReadOut(H, eng, C, S, A, (Hs, Ws), self.n_bands, self.mask_threshold)
        self._ro.alias(self)
        self._H = H
        self._rebuild()
        self.check_render(self.segments["render"][0],
                          "air_parse_render declines a %d x %d scene with %d slots: its LDS carve (the slots' bordered glimpses and "
                          "the axis tables of a band) passes the 160 KiB of a workgroup; use fewer windows or a smaller scene"
                          % (self.scene_size + (self.T,)))
        eng.synchronize()

    def rows(self):
        """the provider protocol (stage.py): the merged, lifted rows of the scenes; a scene has no count posterior"""
        return compacted_rows(self, None, self.scenes)

    # ---- the launches around the provider's own call -------------------------------------------------------------------------
    def _build_plan(self):
        H, eng, par, rows, ro = self._H, self.engine, self.provider, self._rows, self._ro
        cfg = eng.cfg
        L, p = H.lib(), H._p
        S, A, T = self.R, int(cfg.n_appearance), self.window_T
        (Hi, Wi), (hc, wc), (Hs, Ws), (sy, sx) = cfg.img_size, cfg.crop_size, self.scene_size, self.stride
        self.segments = OrderedDict([
            ("gather", [(L.air_tile_gather, (p(self.scenes), S, Hs, Ws, Hi, Wi, sy, sx, p(self.windows)), "air_tile_gather")]),
            ("merge", [(L.air_tile_merge,
                        (p(rows["what"]), p(rows["where"]), p(rows["glimpse"]), p(par.score), p(par.num_objects), T, S, A, hc * wc,
                         Hs, Ws, Hi, Wi, sy, sx, self.iou_merge, p(self.what), p(self.where), p(self.glimpse), p(self.score_src),
                         p(self.kept_cand), p(self.num_objects_in), p(self.cand_state), p(self.dup_of), p(self.merge_counts)),
                        "air_tile_merge")]),
            ("objects", [ro.objects(None, self.num_objects_in, self.where, self.what)]),
            ("relabel", [ro.relabel("air_tile_relabel", self.score_src, self.kept_cand)]),
            ("render", [ro.render(self.glimpse, self.where, self.scenes)]),
            ("rec_sum", [ro.rec_sum()])])
        self._plan = [e for name, seg in self.segments.items() if name != "gather" for e in seg]

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call around the bound provider's own (`parser` holds that provider's launch_count())"""
        return {"tile_gather": 1, "parser": self.provider.launch_count(), "tile_merge": 1, "parse_objects": 1, "tile_relabel": 1,
                "parse_render": 1, "rec_sum": 1}

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def stage(self, scenes):
        """copy the caller's scenes [S, Hs, Ws] (or [S, Hs * Ws]) into the object's own buffer, on the engine's stream"""
        import torch
        eng, S = self.engine, self.R
        scenes = torch.as_tensor(scenes)
        if scenes.shape[0] != S or scenes.numel() != self.scenes.numel():
            raise ValueError("expected %d scenes of %d x %d pixels, got %s" % ((S,) + self.scene_size + (tuple(scenes.shape),)))
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            self.scenes.copy_(scenes.reshape(self.scenes.shape), non_blocking=True)
        if scenes.is_cuda:
            scenes.record_stream(eng.stream)

    def run_provider(self, *args, **kwargs):
        """the bound provider's `parse()` on the gathered windows (further arguments go to it unchanged)"""
        par, rows = self.provider, self._rows
        (Hi, Wi) = self.engine.cfg.img_size
        base = par.parse(self.windows.view(-1, Hi, Wi), *args, **kwargs)
        self.check_same_buffers(base, dict({k: rows[k] for k in ("what", "where", "glimpse")}, score=par.score,
                                           num_objects=par.num_objects), "tiled parser", bound="provider")
        return base

    def parse(self, scenes, *args, **kwargs):
        """scenes [S, Hs, Ws] (or [S, Hs * Ws]); further arguments go to the provider's `parse()` unchanged.  Returns device tensors
        that the NEXT call overwrites.  With scene meaning, at T := C slots and R := S scenes: num_objects [S] int32, presence, score
        [C, S] (the windows' per-step scores), boxes [C, S, 4] (scene pixels), what [C, S, A], where [C, S, 4] (scene frame), glimpse
        [C, S, h, w], offsets, obj_image, obj_step (the candidate id c: c // T_window is the window), obj_box, obj_score, obj_where,
        obj_what, reconstruction [S, Hs, Ws], rec [S], owner [S, Hs, Ws] int8, area [C, S] int32 -- there is no count_prob of a scene;
        of the merge: kept_cand [C, S] int32 (-1 beyond the count), cand_state [S, Nc] int8, dup_of [S, Nc] int32, merge_counts
        [S, 6] int32 (absent, kept, not owned, duplicate, overflow, non-finite);  windows [S * Nw, H, W];  window_num_objects and
        window_count_prob [S, Nw]: the provider's.  Same stream contract as the parsers."""
        eng = self.engine
        self._refresh_plan()
        self.stage(scenes)
        eng._run(self.segments["gather"], eng._sp())
        base = self.run_provider(*args, **kwargs)
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        return self.result(base)

    def result(self, base=None):
        cfg, S, Nw = self.engine.cfg, self.R, self.n_windows
        out = self._ro.result(self.glimpse)
        del out["count_prob"]                                      # (there is no count posterior of a scene)
        out.update({"what": self.what, "where": self.where, "kept_cand": self.kept_cand, "cand_state": self.cand_state,
                    "dup_of": self.dup_of, "merge_counts": self.merge_counts, "windows": self.windows.view(S * Nw, *cfg.img_size)})
        if base is not None:
            out["window_num_objects"] = base["num_objects"].view(S, Nw)
            out["window_count_prob"] = base["count_prob"].view(S, Nw)
        return out
