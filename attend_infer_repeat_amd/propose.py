"""Proposing missed objects from the residual image behind a scene parse: "attend, infer, repeat" applied once more.

Every parse so far -- the mode, best of K, gradient refinement, the exact subset MAP of prune.py -- can only keep, move or drop the T
steps the one forward pass computed.  When the inference network put two steps on one object, or stopped early, nothing downstream can
find the object it never looked at.  The model can look again: subtract what the current parse explains, show the inference network
what is left, and let the generative model decide -- by the same exact arg-max of log p(x, z_S) the pruner uses -- whether the new
steps belong in the scene.  One round, on the `current rows` (round 0: the provider's start rows; later: the first T rows the previous
round left):

  1. residual   res = clamp(x - mult * canvas of the rows t < n_b) into [0, clamp_hi], x always the ORIGINAL image;
  2. forward    the engine's forward plan at the mode on res, from the fresh initial state: its steps 0 .. P-1 are the proposals
                (what, where, raw glimpse, and as score the step weight of that pass; its presence chain does not gate them);
  3. pool       C = T + P <= 6 candidate rows: the T current rows, then the P proposals (bit copies), pool_presence = the current
                chain, pool_source = where every row came from, pool_prior = the count table followed by zeros, so a subset of more
                than T rows has log pi = -inf, never beats the start strictly, and the selected count stays <= T;
  4. search     air_prune_score / air_prune_select unchanged, with T := C, every row a candidate, obs = the original image;
  5. source     source_out[j] = pool_source[kept_step[j]].

The kept count is <= T, so the first T rows of the compacted [C, B, .] outputs hold every kept row; they are the next round's current
rows, and after the last round the read-out the pruner has (air_parse_objects in its given-counts form with the START parse's
presence_prob, air_prune_relabel with source_out as the labels, air_parse_render, air_sum_leading).  What follows: the objective never
decreases over rounds; objective_start of round r + 1 is objective of round r bit for bit (the compaction keeps step order, so canvas
and latent terms are added in the same order); an image whose every round keeps its start mask returns the provider's parse bit for bit.

`ParseProposer` binds to the providers the pruner binds to (parse.SceneParser, particle_parse.ParticleParser, refine.ParseRefiner)
and owns a B-row SceneParser whose engine, at the mode, runs the proposal pass: the provider's rows and image are never overwritten
and a K * B-row particle engine is no special case.  That engine's forward plan entries are launched on the PROVIDER's engine stream;
the whole list -- all rounds and the read-out -- is ONE hipGraph after `capture()`.  New entries of libair_hip.so (include/air_hip.h):
air_propose_residual (the hot path: parse_render_kernel's staging, but it writes the residual and nothing else), air_propose_pool,
air_propose_source (a launch of its own: it runs behind the search, the pool in front of it).

Limits: T + P <= 6; counts above T, re-refining the latents after a proposal was accepted and a refiner chained behind the proposer
are out of scope; a shift prior given without `loc` is refused, because the compaction does not carry where_loc rows.
`reference_residual` and `reference_pool` restate the two kernels in numpy float64 / as plain copies; the search is
prune.reference_score / prune.reference_select.
"""
import ctypes
from typing import Dict

from . import prune
from .engine_config import EngineConfig
from .launch import destroy_graphs

MAX_POOL = prune.MAX_STEPS                                         # air_prune_score is instantiated up to 6 rows
SEGMENTS = ("residual", "forward", "pool", "score", "select", "source")


def check_arguments(cfg: EngineConfig, proposals: int = 1, rounds: int = 1) -> None:
    """Refuse what cannot be proposed this way (pure host code: importable and callable without a GPU)."""
    prune.check_arguments(cfg, "all")
    T, P = int(cfg.max_steps), int(proposals)
    if P < 1 or P > T:
        raise ValueError("proposals: between 1 and max_steps = %d proposal steps per round (the proposal pass computes max_steps "
                         "steps), got %r" % (T, proposals))
    if T + P > MAX_POOL:
        raise ValueError("the candidate pool holds max_steps + proposals rows and the subset search stops at %d rows: "
                         "max_steps + proposals <= %d, got %d + %d" % (MAX_POOL, MAX_POOL, T, P))
    if int(rounds) < 1:
        raise ValueError("rounds must be >= 1, got %r" % (rounds,))
    if cfg.where_shift_prior[0] is None:
        raise ValueError("proposing needs where_shift_prior with a `loc`: a shift prior centred on where_loc needs the where_loc row "
                         "of every pool row, and the compaction does not carry them")


def reference_residual(glimpse, where, n, obs, mult, clamp_hi=1.0):
    """air_propose_residual restated in plain numpy float64: glimpse [T, B, h, w], where [T, B, 4], n [B] (rows t < n[b] are in the
    canvas), obs [B, H, W].  Returns (res [B, H, W], energy [B] = sum res^2)."""
    import numpy as np
    glimpse, where, obs = np.asarray(glimpse, np.float64), np.asarray(where, np.float64), np.asarray(obs, np.float64)
    T, B = glimpse.shape[:2]
    H, W = obs.shape[1:]
    canvas = np.zeros((B, H, W))
    for t in range(T):                                             # step order from 0
        layer = prune._st_write(glimpse[t], where[t], (H, W))
        live = (t < np.asarray(n))[:, None, None]
        canvas = np.where(live, canvas + layer, canvas)
    with np.errstate(invalid="ignore", over="ignore"):
        d = obs - mult * canvas
        res = np.where(d > 0, np.minimum(d, clamp_hi), 0.0)        # a NaN compares false: 0
    return res, (res * res).reshape(B, -1).sum(1)


def reference_pool(what, where, glimpse, score, n, prop_what, prop_where, prop_glimpse, prop_score, prior, proposals, round=0,
                   source_in=None):
    """air_propose_pool as plain copies.  Current rows what [T, B, A], where [T, B, 4], glimpse [T, B, G], score [T, B], n [B]; the
    proposals are rows 0 .. P-1 of the prop_* arrays; prior [T+1].  Returns what / where / glimpse / score [C, B, .] (the inputs'
    dtype), presence [C, B] float32, source [C, B] int32, prior [C+1] float64."""
    import numpy as np
    T, B = np.shape(score)
    P = int(proposals)
    C = T + P
    cat = lambda a, b: np.concatenate([np.asarray(a)[:T], np.asarray(b)[:P]], 0)
    src = np.empty((C, B), np.int32)
    src[:T] = np.arange(T)[:, None] if source_in is None else np.asarray(source_in)[:T]
    src[T:] = (T + int(round) * P + np.arange(P))[:, None]
    n = np.clip(np.asarray(n), 0, T)
    return {"what": cat(what, prop_what), "where": cat(where, prop_where), "glimpse": cat(glimpse, prop_glimpse),
            "score": cat(score, prop_score), "presence": (np.arange(C)[:, None] < n[None, :]).astype(np.float32), "source": src,
            "prior": np.concatenate([np.asarray(prior, np.float64)[:T + 1], np.zeros(P)])}


def reference_source(pool_source, kept_step):
    """air_propose_source: source_out[j, b] = pool_source[kept_step[j, b], b]"""
    import numpy as np
    pool_source, kept_step = np.asarray(pool_source), np.asarray(kept_step)
    return np.take_along_axis(pool_source, kept_step.astype(np.int64), 0).astype(np.int32)


class ParseProposer:
    def __init__(self, parser, proposals: int = 1, rounds: int = 1, clamp_hi: float = 1.0, normalize_steps_prior: bool = True):
        cfg = parser.engine.cfg
        check_arguments(cfg, proposals, rounds)
        import torch
        from . import hip as H
        from .parse import SceneParser
        self.parser, self.engine = parser, parser.engine
        self.proposals, self.rounds, self.clamp_hi = int(proposals), int(rounds), float(clamp_hi)
        self.normalize_steps_prior = bool(normalize_steps_prior)
        self.T, self.R = parser.T, parser.R
        self.C = self.T + self.proposals
        self.mask_threshold = parser.mask_threshold
        eng, dev = self.engine, self.engine.device
        T, B, A, P, C, Rn = self.T, self.R, int(cfg.n_appearance), self.proposals, self.C, self.rounds
        (Hi, Wi), hw = cfg.img_size, cfg.n_crop
        NM = 1 << C
        # the proposal pass: a B-row engine at the mode, built as SceneParser builds its own
        self.proposal = SceneParser(cfg, B, device=dev, mask_threshold=self.mask_threshold)
        self.n_bands = int(H.lib().air_canvas_unroll_bands(B, int(Hi)))
        self._start = prune._start_buffers(parser)
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.res_parts, self.residual_energy = z((Rn, self.n_bands, B)), z((Rn, B))
            self.pool_what, self.pool_where, self.pool_glimpse = z((Rn, C, B, A)), z((Rn, C, B, 4)), z((Rn, C, B, hw))
            self.pool_score, self.pool_presence = z((Rn, C, B)), z((Rn, C, B))
            # every round has its own pool, joint table and compacted rows; pool_prior is ONE buffer, not per-round state: every
            # round's air_propose_pool rewrites it with the same values (the count table followed by zeros)
            self.pool_source, self.pool_prior = z((Rn, C, B), torch.int32), z((C + 1,), torch.float64)
            self.rec_sub = z((Rn, self.n_bands, B, NM))
            self.J_sub = torch.full((Rn, B, NM), float("nan"), dtype=torch.float64, device=dev)
            self.best_mask, self.num_objects_round = z((Rn, B), torch.int32), z((Rn, B), torch.int32)
            self.kept_pool = z((Rn, C, B), torch.int32)
            self.objective_rounds, self._objective_start = z((Rn + 1, B), torch.float64), z((Rn, B), torch.float64)
            self.evidence = z((Rn, C, B), torch.float64)
            self.out_what, self.out_where, self.out_glimpse = z((Rn, C, B, A)), z((Rn, C, B, 4)), z((Rn, C, B, hw))
            self.out_score, self.source_out = z((Rn, C, B)), z((Rn, C, B), torch.int32)
            # the read-out of the last round's first T rows (what the parsers keep)
            self.what, self.where, self.glimpse = self.out_what[-1, :T], self.out_where[-1, :T], self.out_glimpse[-1, :T]
            self.score_src, self.kept_step = self.out_score[-1, :T], self.source_out[-1, :T]
            self.num_objects_in = self.num_objects_round[-1]
            self.num_objects, self.count_prob = z((B,), torch.int32), z((B,))
            self.presence, self.score, self.boxes = z((T, B)), z((T, B)), z((T, B, 4))
            self.offsets = z((B + 1,), torch.int32)
            self.obj_image, self.obj_step = z((T * B,), torch.int32), z((T * B,), torch.int32)
            self.obj_box, self.obj_score = z((T * B, 4)), z((T * B,))
            self.obj_where, self.obj_what = z((T * B, 4)), z((T * B, A))
            self.reconstruction = z((B, Hi, Wi))
            self.rec_parts, self.rec = z((self.n_bands, B)), z((B,))
            self.owner = z((B, Hi, Wi), torch.int8)
            self.area = z((T, B), torch.int32)
        self.objective_start_rounds = [self.objective_rounds[0]] + [self._objective_start[r] for r in range(1, Rn)]
        self.residual = self.proposal.engine.obs.view(B, Hi, Wi)
        self._graph = None
        self._H = H
        self._build_plan()
        eng.synchronize()
        self.proposal.engine.synchronize()

    # ---- the launches behind the provider's own call -------------------------------------------------------------------------
    def _build_plan(self):
        H, eng, par, st, ieng = self._H, self.engine, self.parser, self._start, self.proposal.engine
        cfg = eng.cfg
        check_arguments(cfg, self.proposals, self.rounds)
        L, p, size = H.lib(), H._p, ctypes.c_size_t
        T, B, A, P, C = self.T, self.R, int(cfg.n_appearance), self.proposals, self.C
        (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
        G = hc * wc
        mult, std = float(cfg.output_multiplier), float(cfg.output_std)
        priors = (float(cfg.what_prior[0]), float(cfg.what_prior[1]), float(cfg.where_scale_prior[0]), float(cfg.where_scale_prior[1]),
                  float(cfg.where_shift_prior[0]), float(cfg.where_shift_prior[1]))
        norm = 1 if self.normalize_steps_prior else 0
        self.segments = []                                         # per round: {name: launch list}, the names of SEGMENTS
        for r in range(self.rounds):
            if r == 0:
                cur = dict(what=st["what"], where=st["where"], glimpse=st["glimpse"], score=par.score)
                presence, n_in, src_in = p(par.presence), None, None
            else:
                cur = dict(what=self.out_what[r - 1], where=self.out_where[r - 1], glimpse=self.out_glimpse[r - 1],
                           score=self.out_score[r - 1])
                presence, n_in, src_in = None, p(self.num_objects_round[r - 1]), p(self.source_out[r - 1])
            start_out = self.objective_rounds[0] if r == 0 else self._objective_start[r]
            seg = {
                "residual": [
                    (L.air_propose_residual,
                     (p(cur["glimpse"]), p(cur["where"]), presence, n_in, p(st["obs"]), mult, self.clamp_hi, T, B, Hi, Wi, hc, wc,
                      self.n_bands, p(ieng.obs), p(self.res_parts[r])), "air_propose_residual"),
                    (L.air_sum_leading, (p(self.res_parts[r]), p(self.residual_energy[r]), self.n_bands, size(B)), "air_sum_leading")],
                "forward": list(ieng._plan_fwd),
                "pool": [
                    (L.air_propose_pool,
                     (p(cur["what"]), p(cur["where"]), p(cur["glimpse"]), p(cur["score"]), presence, n_in, src_in, p(ieng.what),
                      p(ieng.where), p(ieng.gd.out[-1]), p(ieng.step_w), p(eng.prior_dev), r, T, P, B, A, G, p(self.pool_what[r]),
                      p(self.pool_where[r]), p(self.pool_glimpse[r]), p(self.pool_score[r]), p(self.pool_presence[r]),
                      p(self.pool_source[r]), p(self.pool_prior)), "air_propose_pool")],
                "score": [
                    (L.air_prune_score,
                     (p(self.pool_glimpse[r]), p(self.pool_where[r]), p(self.pool_presence[r]), p(st["obs"]), mult, std, 1, C, B, Hi,
                      Wi, hc, wc, self.n_bands, p(self.rec_sub[r])), "air_prune_score")],
                "select": [
                    (L.air_prune_select,
                     (p(self.pool_what[r]), p(self.pool_where[r]), p(self.pool_glimpse[r]), p(self.pool_score[r]),
                      p(self.pool_presence[r]), None, *priors, p(self.pool_prior), norm, 1, p(self.rec_sub[r]), self.n_bands, C, B, A,
                      G, p(self.J_sub[r]), p(self.best_mask[r]), p(self.num_objects_round[r]), p(self.kept_pool[r]),
                      p(self.objective_rounds[r + 1]), p(start_out), p(self.evidence[r]), p(self.out_what[r]), p(self.out_where[r]),
                      p(self.out_glimpse[r]), p(self.out_score[r])), "air_prune_select")],
                "source": [
                    (L.air_propose_source, (p(self.pool_source[r]), p(self.kept_pool[r]), C, B, p(self.source_out[r])),
                     "air_propose_source")]}
            self.segments.append(seg)
        self.readout = [
            (L.air_parse_objects,
             (p(st["presence_prob"]), p(self.num_objects_in), p(self.where), p(self.what), T, B, A, Hi, Wi, p(self.num_objects),
              p(self.count_prob), p(self.presence), p(self.score), p(self.boxes), p(self.offsets), p(self.obj_image), p(self.obj_step),
              p(self.obj_box), p(self.obj_score), p(self.obj_where), p(self.obj_what)), "air_parse_objects"),
            (L.air_prune_relabel,
             (p(self.score_src), p(self.kept_step), p(self.num_objects), p(self.offsets), T, B, p(self.score), p(self.obj_score),
              p(self.obj_step)), "air_prune_relabel"),
            (L.air_parse_render,
             (p(self.glimpse), p(self.where), p(self.presence), p(st["obs"]), mult, std, self.mask_threshold, T, B, Hi, Wi, hc, wc,
              self.n_bands, p(self.reconstruction), p(self.rec_parts), p(self.owner), p(self.area), None), "air_parse_render"),
            (L.air_sum_leading, (p(self.rec_parts), p(self.rec), self.n_bands, size(B)), "air_sum_leading")]
        self._plan = [e for seg in self.segments for name in SEGMENTS for e in seg[name]] + self.readout
        self._built_for = self._plan_key()
        self._built_on = ieng._plan_fwd

    def _plan_key(self):
        """what of the engine's configuration the launch list holds by value"""
        cfg = self.engine.cfg
        return (cfg.output_multiplier, cfg.output_std, cfg.what_prior, cfg.where_scale_prior, cfg.where_shift_prior)

    def _refresh_plan(self):
        """rebuild (and re-capture) when a switch of the provider's engine moved without the proposer being told, or the proposal
        engine rebuilt its forward plan"""
        if self._plan_key() == self._built_for and self.proposal.engine._plan_fwd is self._built_on:
            return False
        had = self._graph is not None
        self.release_graphs()
        self._build_plan()
        if had:
            self.capture()
        return True

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call behind the bound provider's own (`parser` holds that provider's launch_count()); the
        per-round entries are counted over all rounds"""
        n = self.rounds
        return {"parser": self.parser.launch_count(), "propose_residual": n, "residual_sum": n,
                "forward": n * len(self.proposal.engine._plan_fwd), "propose_pool": n, "prune_score": n, "prune_select": n,
                "propose_source": n, "parse_objects": 1, "prune_relabel": 1, "parse_render": 1, "rec_sum": 1}

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def load_from(self, train_engine):
        """device-to-device copy of another engine's parameters into the bound provider's engine AND the proposal engine, its step
        counter (the count prior pi depends on it) and run-time switches"""
        from . import iw_eval
        iw_eval.load_inner_engine(self, train_engine)
        self.proposal.load_from(train_engine)
        self._refresh_plan()

    def load_parameters(self, named):
        self.parser.load_parameters(named)
        self.proposal.load_parameters(named)

    def set_global_step(self, step: int):
        self.parser.set_global_step(step)
        self.proposal.set_global_step(step)

    def update_config(self, **changes) -> bool:
        """run-time switches of both engines (AIREngine.KNOBS): the provider re-captures its graphs, the proposer rebuilds its launch
        list (output_multiplier is one of its arguments, the proposal engine's forward plan a part of it) and re-captures when one
        changed"""
        if self._graph is not None:
            self.engine.synchronize()
        changed = self.parser.update_config(**changes)
        changed = self.proposal.update_config(**changes) or changed
        return self._refresh_plan() or changed

    # ---- graphs -------------------------------------------------------------------------------------------------------------
    def capture(self):
        """every launch behind the provider's own call -- all rounds and the read-out -- as ONE hipGraph (the provider's graphs are its
        own: `parser.capture()`)"""
        self.release_graphs()
        self.engine.synchronize()
        self.proposal.engine.synchronize()
        self._graph = self.engine._capture_plans([self._plan])

    def release_graphs(self):
        destroy_graphs([self._graph])
        self._graph = None

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def _order_engines(self, before: bool):
        """the proposal engine's forward plan runs on the provider's stream: that stream follows whatever the proposal engine's own
        stream still has pending (parameter loads), and the other way round afterwards"""
        a, b = self.engine.stream, self.proposal.engine.stream
        if before:
            a.wait_stream(b)
        else:
            b.wait_stream(a)

    def parse(self, obs, *args, **kwargs):
        """The bound provider's `parse(obs, ...)` (further arguments go to it unchanged), then the rounds and the read-out.  Returns
        device tensors that the NEXT call overwrites: every key of the provider's result and of ParsePruner.parse with the same
        meaning -- num_objects, count_prob, presence, score, boxes, what, where, glimpse, the object table, reconstruction, rec, owner,
        area describe the parse after the last round (row j is pool row kept_step[j]); presence_prob, num_steps_posterior and a
        provider's other read-outs are the provider's; objective / objective_start [B] float64 are J after the last round / of the
        start parse; objective_subsets [B, 2^C], best_mask [B] and evidence [C, B] are the LAST round's, over its pool;
        kept_step [T, B] int32 is source_out: a value < T is a start step, T + r * P + j is proposal j of round r -- and
          objective_rounds [rounds + 1, B] float64 (row 0: the start, row r + 1: after round r), residual [B, H, W] (the last round's),
          residual_energy [rounds, B], proposal_what / proposal_where / proposal_glimpse / proposal_score [rounds, P, B, .],
          num_objects_start [B] int32, objects_proposed_kept [B] int32 (objects of the result that came from a proposal);
        behind a ParseRefiner also refine_objective, refine_objective_start.  Same stream contract as the parsers."""
        eng, par, st = self.engine, self.parser, self._start
        self._refresh_plan()
        base = par.parse(obs, *args, **kwargs)
        for k in ("what", "where", "glimpse", "presence_prob"):
            if base[k].data_ptr() != st[k].data_ptr():
                raise RuntimeError("the bound parser returned %r from another buffer than the proposer was built on" % k)
        for k in ("presence", "score", "num_objects"):
            if base[k].data_ptr() != getattr(par, k).data_ptr():
                raise RuntimeError("the bound parser returned %r from another buffer than the proposer was built on" % k)
        self._order_engines(True)
        eng._replay_or_run(self._graph, self._plan)
        self._order_engines(False)
        eng.wait_for_engine()
        return self._result(base)

    def _result(self, base):
        import torch
        cfg, T, B, P = self.engine.cfg, self.T, self.R, self.proposals
        out = dict(base)
        if "best_iter" in base:                                    # behind a refiner: its objectives keep a name of their own
            out["refine_objective"], out["refine_objective_start"] = base["objective"], base["objective_start"]
        with torch.cuda.device(self.engine.device):
            proposed = ((self.kept_step >= T) & (self.presence > 0.5)).sum(0).to(torch.int32)
        out.update({"num_objects": self.num_objects, "count_prob": self.count_prob, "presence": self.presence, "score": self.score,
                    "boxes": self.boxes, "what": self.what, "where": self.where,
                    "glimpse": self.glimpse.view(T, B, *cfg.crop_size), "offsets": self.offsets,
                    "obj_image": self.obj_image, "obj_step": self.obj_step, "obj_box": self.obj_box, "obj_score": self.obj_score,
                    "obj_where": self.obj_where, "obj_what": self.obj_what, "reconstruction": self.reconstruction, "rec": self.rec,
                    "owner": self.owner, "area": self.area, "objective": self.objective_rounds[-1],
                    "objective_start": self.objective_rounds[0], "objective_subsets": self.J_sub[-1], "best_mask": self.best_mask[-1],
                    "kept_step": self.kept_step, "evidence": self.evidence[-1], "num_objects_start": self.parser.num_objects,
                    "objective_rounds": self.objective_rounds, "residual": self.residual, "residual_energy": self.residual_energy,
                    "proposal_what": self.pool_what[:, T:], "proposal_where": self.pool_where[:, T:],
                    "proposal_glimpse": self.pool_glimpse[:, T:].view(self.rounds, P, B, *cfg.crop_size),
                    "proposal_score": self.pool_score[:, T:], "objects_proposed_kept": proposed})
        out.pop("layers", None)                                    # (the provider's layers are the start parse's)
        return out

    def synchronize(self):
        self.engine.synchronize()
