"""Letting a scene parse change its count on the device: the exact arg-max of log p(x, z_S) over the subsets S of the T computed steps.

    log p(x, z_S) = log p(x | mult * sum_{t in S} layer_t) + sum_{t in S} log p(z_t) + log pi(|S|)

The canvas is a sum and the per-step priors are i.i.d., so the joint is defined for every subset of steps, not only for the leading-
ones chains the inference network emits; with T <= 6 there are at most 64 subsets and the discrete problem refine.py leaves open
("the count stays fixed") is solved by enumeration -- one pass over the pixels for all subsets.  The forward pass computes latents and
glimpses of all T steps, so the enumeration may also switch ON a step the presence chain declined (candidates="all").

A subset is a mask m, bit t = step t is kept.  Per image: n = the number of leading ones of the start parse's presence, the candidate
steps are t < c with c = n ("present": objects can only be removed) or c = T ("all"), the start mask is m0 = 2^n - 1.  m0 is visited
first and always taken, then every other mask from 2^c - 1 down to 0; a mask replaces the best one iff its J is not NaN and (the best
is NaN or J > best), strictly: the parse is unchanged on a tie, never worse than the start, unchanged when everything is NaN.
evidence[t] = J(m0 with bit t) - J(m0 without bit t): how much the model wants object t, a ranking figure of its own.

`ParsePruner` owns no engine: it binds to a parse.SceneParser, a particle_parse.ParticleParser or a refine.ParseRefiner, runs that
provider's own `parse()` and then, on the same engine stream, its own launch list of libair_hip.so entries (include/air_hip.h), captured
as ONE hipGraph by `capture()`:

  air_prune_score    the reconstruction term of every mask in row bands (the hot path);
  air_prune_select   the latent terms, J of every mask in float64, the arg-max, the evidence, and the rows compacted into a
                     leading-ones chain (a stable partition: kept steps in step order, then the others; bit copies);
  air_parse_objects  (given counts) on the compacted rows, with the start parse's presence_prob: count_prob = q(n');
  air_prune_relabel  score / obj_score / obj_step of the kept rows: air_parse_objects labels rows by position;
  air_parse_render, air_sum_leading   reconstruction, rec, owner, area of the selected subset.

One exception to "one hipGraph", the one refine.py has: behind a ParticleParser with a shift prior given without `loc`, particle 0's
where_loc rows are gathered by a strided device copy on the engine stream BEFORE the launch list.

This closes "the count stays fixed" only for subsets of the T computed steps; proposing new objects from a residual image stays open.
`reference_score` and `reference_select` restate the two kernels in numpy float64.
"""
import math
from typing import Dict

from . import iw_eval
from .engine_config import EngineConfig
from .stage import BoundStage, ReadOut, compacted_rows, prior_arguments

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
MAX_STEPS = 6                      # air_prune_score is instantiated for T = 1 .. 6: at most 64 subsets
CANDIDATES = {"present": 0, "all": 1}


def check_arguments(cfg: EngineConfig, candidates: str = "present") -> None:
    """Refuse what cannot be pruned this way (pure host code: importable and callable without a GPU).  The priors are needed: they
    are the latent terms of log p(x, z).  bf16 MLPs are fine: nothing here runs the decoder."""
    if candidates not in CANDIDATES:
        raise ValueError('candidates must be "present" or "all", got %r' % (candidates,))
    if int(cfg.max_steps) > MAX_STEPS:
        raise ValueError("subset pruning enumerates every subset of the computed steps and stops at 64 subsets: max_steps <= %d, "
                         "got %d" % (MAX_STEPS, int(cfg.max_steps)))
    iw_eval.check_config(cfg, 1)


def _st_write(glimpse, where, img):
    """float64 inverse spatial-transformer write of one step: glimpse [B, h, w], where [B, 4] = [sx, tx, sy, ty] -> [B, H, W]
    (the taps and the bilinear form of air_parse_render; a tap outside the glimpse is zero, a coordinate outside (-1, extent) gives 0)"""
    import numpy as np
    B, h, w = glimpse.shape
    H, W = img
    out = np.zeros((B, H, W))
    X, Y = np.linspace(-1.0, 1.0, W), np.linspace(-1.0, 1.0, H)
    if W == 1:
        X = np.array([-1.0])
    if H == 1:
        Y = np.array([-1.0])
    pad = np.zeros((B, h + 2, w + 2))
    pad[:, 1:-1, 1:-1] = glimpse
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            sx, tx, sy, ty = where[b]
            cx = ((1.0 / sx) * X + (-tx / sx) + 1.0) * ((w - 1) / 2.0)
            cy = ((1.0 / sy) * Y + (-ty / sy) + 1.0) * ((h - 1) / 2.0)
            vx, vy = (cx > -1.0) & (cx < w), (cy > -1.0) & (cy < h)
            fx = np.where(vx, np.floor(np.where(vx, cx, 0.0)), 0.0).astype(np.int64)
            fy = np.where(vy, np.floor(np.where(vy, cy, 0.0)), 0.0).astype(np.int64)
            dx, dy = (fx + 1.0) - np.where(vx, cx, 0.0), (fy + 1.0) - np.where(vy, cy, 0.0)
            g = pad[b]
            iy, ix = fy[:, None] + 1, fx[None, :] + 1
            DX, DY = dx[None, :], dy[:, None]
            val = (DX * DY) * g[iy, ix] + ((1 - DX) * (1 - DY)) * g[iy + 1, ix + 1] + (DX * (1 - DY)) * g[iy + 1, ix] \
                + ((1 - DX) * DY) * g[iy, ix + 1]
            out[b] = np.where(vy[:, None] & vx[None, :], val, 0.0)
    return out


def leading_ones(presence):
    import numpy as np
    return np.cumprod(np.asarray(presence) > 0.5, axis=0).sum(0).astype(np.int64)


def reference_score(glimpse, where, presence, obs, mult, std, all_candidates, layers=None):
    """air_prune_score restated in plain numpy float64 (include/air_hip.h states the rule), summed over the bands: glimpse [T, B, h, w],
    where [T, B, 4], presence [T, B], obs [B, H, W].  `layers` [T, B, H, W]: float64 st_write layers computed elsewhere, used instead
    of this module's own inverse warp.  Returns rec_sub [B, 2^T] float64, NaN for the masks m >= 2^c that the kernel does not write."""
    import numpy as np
    glimpse, where, obs = np.asarray(glimpse, np.float64), np.asarray(where, np.float64), np.asarray(obs, np.float64)
    T, B = glimpse.shape[:2]
    H, W = obs.shape[1:]
    n = leading_ones(presence)
    c = np.full(B, T) if all_candidates else n
    if layers is None:
        layers = np.stack([_st_write(glimpse[t], where[t], (H, W)) for t in range(T)], 0)
    layers = np.asarray(layers, np.float64)
    out = np.full((B, 1 << T), np.nan)
    cst = HALF_LOG_2PI + math.log(std)
    for m in range(1 << T):
        canvas = np.zeros((B, H, W))
        for t in range(T):                                         # step order from 0
            if (m >> t) & 1:
                canvas = canvas + layers[t]
        with np.errstate(invalid="ignore", over="ignore"):
            z = (obs - mult * canvas) / std
            rec = (0.5 * z * z + cst).reshape(B, -1).sum(1)
        live = m < (1 << c)
        out[live, m] = rec[live]
    return out


def _log_normal(x, loc, scale):
    import numpy as np
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = (x - loc) / scale
        return -0.5 * z * z - np.log(scale) - HALF_LOG_2PI


def select_masks(J_sub, n, T, all_candidates):
    """the visiting rule on a table of joints J_sub [B, 2^T] (any float dtype; compared as float64): returns best_mask [B] int64"""
    import numpy as np
    J = np.asarray(J_sub, np.float64)
    best_mask = np.zeros(len(n), np.int64)
    for b in range(len(n)):
        c = T if all_candidates else int(n[b])
        m0 = (1 << int(n[b])) - 1
        bm, best = m0, J[b, m0]                                    # m0 first: always taken
        for m in range((1 << c) - 1, -1, -1):
            if m == m0:
                continue
            v = J[b, m]
            if not math.isnan(v) and (math.isnan(best) or v > best):
                bm, best = m, v
        best_mask[b] = bm
    return best_mask


def partition(mask, T):
    """stable partition of 0 .. T-1: the steps in `mask` in step order, then all other steps in step order"""
    return [t for t in range(T) if (mask >> t) & 1] + [t for t in range(T) if not (mask >> t) & 1]


def reference_select(what, where, glimpse, score, presence, where_loc, priors, prior, normalize_prior, all_candidates, rec_sub,
                     J_sub=None):
    """air_prune_select restated in plain numpy float64.  Arrays as the kernel takes them (what [T, B, A], where [T, B, 4], glimpse
    [T, B, G], score [T, B], presence [T, B], rec_sub [n_bands, B, 2^T] or band-summed [B, 2^T]); priors = (what_loc, what_scale,
    scale_loc, scale_scale, shift_loc or None / NaN, shift_scale); prior = the count table [T+1].  J_sub: a table of joints to run
    the selection, the evidence and the objectives on instead of the one formed here (the device's own, say).  Returns
      lp [T, B], J_sub [B, 2^T] (NaN for m >= 2^c), best_mask, num_objects, n [B], kept_step [T, B], objective, objective_start [B],
      evidence [T, B] (NaN for t >= c), and what / where / glimpse / score compacted (the inputs' dtype: copies)."""
    import numpy as np
    f = lambda a: np.array(a, dtype=np.float64)
    T, B, A = np.shape(what)
    NM = 1 << T
    w_loc, w_scale, s_loc, s_scale, h_loc, h_scale = [float("nan") if v is None else float(v) for v in priors]
    n = leading_ones(presence)
    c = np.full(B, T) if all_candidates else n
    mu = np.empty((T, B, 4))
    mu[..., 0::2] = s_loc
    mu[..., 1::2] = f(where_loc)[..., 1::2] if math.isnan(h_loc) else h_loc
    sd = np.empty((T, B, 4))
    sd[..., 0::2], sd[..., 1::2] = s_scale, h_scale
    lp = _log_normal(f(what), w_loc, w_scale).sum(-1) + _log_normal(f(where), mu, sd).sum(-1)                  # [T, B]
    pi = f(prior)
    total = 1.0
    if normalize_prior:
        total = 0.0
        for v in pi:
            total = total + v
    with np.errstate(divide="ignore", invalid="ignore"):
        log_pi = np.log(pi / total)
    rec = f(rec_sub)
    if rec.ndim == 3:
        acc = np.zeros((B, NM))
        for k in range(rec.shape[0]):
            acc = acc + rec[k]
        rec = acc
    J = np.full((B, NM), np.nan)
    for m in range(NM):
        lat = np.zeros(B)
        for t in range(T):
            if (m >> t) & 1:
                lat = lat + lp[t]
        with np.errstate(invalid="ignore"):
            v = (-rec[:, m] + lat) + log_pi[bin(m).count("1")]
        live = m < (1 << c)
        J[live, m] = v[live]
    own_J = J
    if J_sub is not None:
        J = np.asarray(J_sub, np.float64)
    best = select_masks(J, n, T, all_candidates)
    m0 = (1 << n) - 1
    rows = np.arange(B)
    evidence = np.full((T, B), np.nan)
    for t in range(T):
        with np.errstate(invalid="ignore"):
            e = J[rows, m0 | (1 << t)] - J[rows, m0 & ~(1 << t)]
        evidence[t, t < c] = e[t < c]
    kept = np.array([partition(int(best[b]), T) for b in range(B)], np.int32).T.reshape(T, B)                   # [T, B]
    gather = lambda a: np.stack([np.asarray(a)[kept[:, b], b] for b in range(B)], 1)
    return {"lp": lp, "J_sub": own_J, "best_mask": best, "num_objects": np.array([bin(int(m)).count("1") for m in best], np.int64),
            "n": n, "kept_step": kept, "objective": J[rows, best], "objective_start": J[rows, m0], "evidence": evidence,
            "what": gather(what), "where": gather(where), "glimpse": gather(glimpse), "score": gather(score)}


def score_entry(H, cfg, glimpse, where, presence, obs, all_candidates, T, B, n_bands, rec_sub):
    L, p = H.lib(), H._p
    (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
    return (L.air_prune_score, (p(glimpse), p(where), p(presence), p(obs), float(cfg.output_multiplier), float(cfg.output_std),
                                all_candidates, T, B, Hi, Wi, hc, wc, n_bands, p(rec_sub)), "air_prune_score")


def select_entry(H, cfg, rows, score, presence, where_loc, prior, normalize_prior, all_candidates, rec_sub, n_bands, T, B, out):
    """air_prune_select on the rows (what, where, glimpse); `out` = (J_sub, best_mask, num_objects, kept_step, objective,
    objective_start, evidence, what, where, glimpse, score)"""
    L, p = H.lib(), H._p
    (hc, wc) = cfg.crop_size
    return (L.air_prune_select,
            (p(rows[0]), p(rows[1]), p(rows[2]), p(score), p(presence), p(where_loc), *prior_arguments(cfg), p(prior),
             1 if normalize_prior else 0, all_candidates, p(rec_sub), n_bands, T, B, int(cfg.n_appearance), hc * wc,
             *(p(t) for t in out)), "air_prune_select")


class ParsePruner(BoundStage):
    KIND = "subset"
    ACCEPTS = ("scene", "particle", "refiner")
    KEY_FIELDS = ("output_multiplier", "output_std", "what_prior", "where_scale_prior", "where_shift_prior")

    def __init__(self, parser, candidates: str = "present", normalize_steps_prior: bool = True):
        self._start = self.bind(parser)
        cfg = parser.engine.cfg
        check_arguments(cfg, candidates)
        import torch
        from . import hip as H
        self.parser, self.engine = parser, parser.engine
        self._bound = parser
        self.candidates, self.normalize_steps_prior = candidates, bool(normalize_steps_prior)
        self.T, self.R = parser.T, parser.R
        self.mask_threshold = parser.mask_threshold
        eng, dev = self.engine, self.engine.device
        T, B, A = self.T, self.R, int(cfg.n_appearance)
        (Hi, Wi), hw = cfg.img_size, cfg.n_crop
        NM = 1 << T
        self.n_bands = int(H.lib().air_canvas_unroll_bands(B, int(Hi)))
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.where_loc = self._start["where_loc"] if self._start["where_loc"] is not None else z((T, B, 4))
            self.rec_sub = z((self.n_bands, B, NM))
            self.J_sub = torch.full((B, NM), float("nan"), dtype=torch.float64, device=dev)
            self.best_mask, self.num_objects_in = z((B,), torch.int32), z((B,), torch.int32)
            self.kept_step = z((T, B), torch.int32)
            self.objective, self.objective_start = z((B,), torch.float64), z((B,), torch.float64)
            self.evidence = z((T, B), torch.float64)
            self.what, self.where, self.glimpse, self.score_src = z((T, B, A)), z((T, B, 4)), z((T, B, hw)), z((T, B))
        # the read-out of the selected subset (what the parsers keep)
        self._ro = ReadOut(H, eng, T, B, A, cfg.img_size, self.n_bands, self.mask_threshold)
        self._ro.alias(self)
        self._H = H
        self._rebuild()
        eng.synchronize()

    def rows(self):
        """the provider protocol (stage.py): the compacted rows; presence_prob and the images are the start parse's"""
        return compacted_rows(self, self._start["presence_prob"], self._start["obs"])

    # ---- the launches behind the provider's own call -------------------------------------------------------------------------
    def _build_plan(self):
        H, eng, par, st, ro = self._H, self.engine, self.parser, self._start, self._ro
        cfg = eng.cfg
        check_arguments(cfg, self.candidates)
        T, B, allc = self.T, self.R, CANDIDATES[self.candidates]
        self._plan = [
            score_entry(H, cfg, st["glimpse"], st["where"], par.presence, st["obs"], allc, T, B, self.n_bands, self.rec_sub),
            select_entry(H, cfg, (st["what"], st["where"], st["glimpse"]), par.score, par.presence, self.where_loc, eng.prior_dev,
                         self.normalize_steps_prior, allc, self.rec_sub, self.n_bands, T, B,
                         (self.J_sub, self.best_mask, self.num_objects_in, self.kept_step, self.objective, self.objective_start,
                          self.evidence, self.what, self.where, self.glimpse, self.score_src)),
            ro.objects(st["presence_prob"], self.num_objects_in, self.where, self.what),
            ro.relabel("air_prune_relabel", self.score_src, self.kept_step)] + ro.tail(self.glimpse, self.where, st["obs"])

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call behind the bound provider's own (`parser` holds that provider's launch_count())"""
        return {"parser": self.parser.launch_count(), "prune_score": 1, "prune_select": 1, "parse_objects": 1, "prune_relabel": 1,
                "parse_render": 1, "rec_sum": 1}

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def parse(self, obs, *args, **kwargs):
        """The bound provider's `parse(obs, ...)` (further arguments go to it unchanged), then the subset search.  Returns device
        tensors that the NEXT call overwrites: every key of the provider's result -- num_objects, count_prob, presence, score, boxes,
        what, where, glimpse, the object table, reconstruction, rec, owner, area now describe the selected subset, compacted into a
        leading-ones chain (row j of what / where / glimpse / score is the start parse's row kept_step[j]); presence_prob,
        num_steps_posterior and a provider's other read-outs are the provider's -- and
          objective, objective_start [B] float64 (J of the selected mask / of the start mask), objective_subsets [B, 2^T] float64
          (J of every mask, NaN beyond 2^c), best_mask [B] int32, kept_step [T, B] int32, evidence [T, B] float64 (NaN for t >= c),
          num_objects_start [B] int32;
        behind a ParseRefiner also refine_objective, refine_objective_start: the refiner's objective / objective_start, whose own
        keys now hold the pruner's.
        Same stream contract as the parsers."""
        eng, par = self.engine, self.parser
        self._refresh_plan()
        base = par.parse(obs, *args, **kwargs)
        self.check_parse(base, "pruner")
        self.gather_where_loc()
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        out = dict(base)
        if par.KIND == "refiner":                                  # its objectives keep a name of their own
            out["refine_objective"], out["refine_objective_start"] = base["objective"], base["objective_start"]
        out.update(self._ro.result(self.glimpse))
        out.update({"what": self.what, "where": self.where, "objective": self.objective, "objective_start": self.objective_start,
                    "objective_subsets": self.J_sub, "best_mask": self.best_mask, "kept_step": self.kept_step,
                    "evidence": self.evidence, "num_objects_start": par.num_objects})
        out.pop("layers", None)                                    # (the provider's layers are the start parse's)
        return out


class SubsetSearchRounds:
    """The rounds of a subset search over a candidate pool of C = T + P rows (propose.py, temporal.py): every round's pool, joint table
    and compacted rows, the `score` / `select` / `source` segments that follow the owner's own pool segment, and the last round's first
    T rows as what the read-out takes.  The owner exposes every buffer under the same name (`alias`)."""

    def __init__(self, H, engine, rounds, T, P, B, n_bands):
        import torch
        cfg, dev = engine.cfg, engine.device
        self._H, self.engine, self.rounds, self.T, self.P, self.C, self.B, self.n_bands = H, engine, rounds, T, P, T + P, B, n_bands
        Rn, C, A, hw, NM = rounds, T + P, int(cfg.n_appearance), cfg.n_crop, 1 << (T + P)
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.pool_what, self.pool_where, self.pool_glimpse = z((Rn, C, B, A)), z((Rn, C, B, 4)), z((Rn, C, B, hw))
            self.pool_score, self.pool_presence = z((Rn, C, B)), z((Rn, C, B))
            # every round has its own pool, joint table and compacted rows; pool_prior is ONE buffer, not per-round state: every
            # round's pool entry rewrites it with the same values (the count table followed by zeros)
            self.pool_source, self.pool_prior = z((Rn, C, B), torch.int32), z((C + 1,), torch.float64)
            self.rec_sub = z((Rn, n_bands, B, NM))
            self.J_sub = torch.full((Rn, B, NM), float("nan"), dtype=torch.float64, device=dev)
            self.best_mask, self.num_objects_round = z((Rn, B), torch.int32), z((Rn, B), torch.int32)
            self.kept_pool = z((Rn, C, B), torch.int32)
            self.objective_rounds, self._objective_start = z((Rn + 1, B), torch.float64), z((Rn, B), torch.float64)
            self.evidence = z((Rn, C, B), torch.float64)
            self.out_what, self.out_where, self.out_glimpse = z((Rn, C, B, A)), z((Rn, C, B, 4)), z((Rn, C, B, hw))
            self.out_score, self.source_out = z((Rn, C, B)), z((Rn, C, B), torch.int32)
        # the last round's first T rows: what the read-out takes (and the owner's rows as a provider)
        self.what, self.where, self.glimpse = self.out_what[-1, :T], self.out_where[-1, :T], self.out_glimpse[-1, :T]
        self.score_src, self.kept_step = self.out_score[-1, :T], self.source_out[-1, :T]
        self.num_objects_in = self.num_objects_round[-1]
        self.objective_start_rounds = [self.objective_rounds[0]] + [self._objective_start[r] for r in range(1, Rn)]

    def alias(self, owner):
        for k, v in vars(self).items():
            if k not in ("_H", "engine", "rounds", "T", "P", "C", "B", "n_bands"):
                setattr(owner, k, v)

    def current(self, r, rows, score, presence, counts):
        """what round r's pool entry reads: (what, where, glimpse, score) and, as the entry takes them, the presence chain, the counts
        and the sources -- round 0: the provider's (a chain or counts), later: what round r - 1 left"""
        p = self._H._p
        if r == 0:
            return (rows["what"], rows["where"], rows["glimpse"], score), p(presence), p(counts), None
        return ((self.out_what[r - 1], self.out_where[r - 1], self.out_glimpse[r - 1], self.out_score[r - 1]), None,
                p(self.num_objects_round[r - 1]), p(self.source_out[r - 1]))

    def pool_out(self, r):
        """round r's pool as the pool entries take it: what, where, glimpse, score, presence, source, prior"""
        p = self._H._p
        return tuple(p(t) for t in (self.pool_what[r], self.pool_where[r], self.pool_glimpse[r], self.pool_score[r],
                                    self.pool_presence[r], self.pool_source[r], self.pool_prior))

    def search(self, r, obs, normalize_prior):
        """the segments behind round r's pool: air_prune_score / air_prune_select with T := C and every row a candidate, then
        air_propose_source: source_out[j] = pool_source[kept_pool[j]]"""
        H, cfg, C, B = self._H, self.engine.cfg, self.C, self.B
        L, p = H.lib(), H._p
        start_out = self.objective_rounds[0] if r == 0 else self._objective_start[r]
        return {
            "score": [score_entry(H, cfg, self.pool_glimpse[r], self.pool_where[r], self.pool_presence[r], obs, 1, C, B, self.n_bands,
                                  self.rec_sub[r])],
            "select": [select_entry(H, cfg, (self.pool_what[r], self.pool_where[r], self.pool_glimpse[r]), self.pool_score[r],
                                    self.pool_presence[r], None, self.pool_prior, normalize_prior, 1, self.rec_sub[r], self.n_bands, C, B,
                                    (self.J_sub[r], self.best_mask[r], self.num_objects_round[r], self.kept_pool[r],
                                     self.objective_rounds[r + 1], start_out, self.evidence[r], self.out_what[r], self.out_where[r],
                                     self.out_glimpse[r], self.out_score[r]))],
            "source": [(L.air_propose_source, (p(self.pool_source[r]), p(self.kept_pool[r]), C, B, p(self.source_out[r])),
                        "air_propose_source")]}

    def readout(self, ro, presence_prob, obs):
        """the pruner's read-out on the last round's first T rows, with the START parse's presence_prob"""
        return [ro.objects(presence_prob, self.num_objects_in, self.where, self.what),
                ro.relabel("air_prune_relabel", self.score_src, self.kept_step)] + ro.tail(self.glimpse, self.where, obs)

    def result(self, base, provider, ro, kept_key):
        """the provider's result with the keys of ParsePruner.parse describing the parse after the last round, the rounds' own keys,
        and under `kept_key` the objects of the result that came from beyond the start rows"""
        import torch
        T, P, B, crop = self.T, self.P, self.B, self.engine.cfg.crop_size
        out = dict(base)
        if provider.KIND == "refiner":                             # its objectives keep a name of their own
            out["refine_objective"], out["refine_objective_start"] = base["objective"], base["objective_start"]
        if provider.KIND == "subset":                              # behind a pruner or proposer
            out["provider_objective"], out["provider_objective_start"] = base["objective"], base["objective_start"]
        with torch.cuda.device(self.engine.device):
            kept = ((self.kept_step >= T) & (ro.presence > 0.5)).sum(0).to(torch.int32)
        out.update(ro.result(self.glimpse))
        out.update({"what": self.what, "where": self.where, "objective": self.objective_rounds[-1],
                    "objective_start": self.objective_rounds[0], "objective_subsets": self.J_sub[-1], "best_mask": self.best_mask[-1],
                    "kept_step": self.kept_step, "evidence": self.evidence[-1], "num_objects_start": provider.num_objects,
                    "objective_rounds": self.objective_rounds, "proposal_what": self.pool_what[:, T:],
                    "proposal_where": self.pool_where[:, T:],
                    "proposal_glimpse": self.pool_glimpse[:, T:].view(self.rounds, P, B, *crop),
                    "proposal_score": self.pool_score[:, T:], kept_key: kept})
        out.pop("layers", None)                                    # (the provider's layers are the start parse's)
        return out
