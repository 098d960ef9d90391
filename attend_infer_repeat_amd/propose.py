"""Proposing missed objects from the residual image behind a scene parse: "attend, infer, repeat" applied once more.

Every parse so far -- the mode, best of K, gradient refinement, the exact subset MAP of prune.py -- can only keep, move or drop the T
steps the one forward pass computed.  When the inference network put two steps on one object, or stopped early, nothing downstream can
find the object it never looked at.  The model can look again: subtract what the current parse explains, show the inference network
what is left, and let the generative model decide -- by the same exact arg-max of log p(x, z_S) the pruner uses -- whether the new
steps belong in the scene.  One round, on the `current rows` (round 0: the provider's start rows; later: the first T rows the previous
round left):

  1. residual   res = clamp(x - mult * canvas of the rows t < n_b) into [0, clamp_hi], x always the ORIGINAL image (a NaN pixel of x
                gives exactly 0; clamp_hi = +inf or NaN clamps nothing above: res = max(d, 0));
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
from .stage import BoundStage, ReadOut, compacted_rows

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


class ParseProposer(BoundStage):
    KIND = "subset"
    ACCEPTS = prune.ParsePruner.ACCEPTS
    KEY_FIELDS = prune.ParsePruner.KEY_FIELDS

    def __init__(self, parser, proposals: int = 1, rounds: int = 1, clamp_hi: float = 1.0, normalize_steps_prior: bool = True):
        self._start = self.bind(parser)
        cfg = parser.engine.cfg
        check_arguments(cfg, proposals, rounds)
        import torch
        from . import hip as H
        from .parse import SceneParser
        self.parser, self.engine = parser, parser.engine
        self._bound = parser
        self.proposals, self.rounds, self.clamp_hi = int(proposals), int(rounds), float(clamp_hi)
        self.normalize_steps_prior = bool(normalize_steps_prior)
        self.T, self.R = parser.T, parser.R
        self.C = self.T + self.proposals
        self.mask_threshold = parser.mask_threshold
        eng, dev = self.engine, self.engine.device
        T, B, Rn = self.T, self.R, self.rounds
        (Hi, Wi) = cfg.img_size
        # the proposal pass: a B-row engine at the mode, built as SceneParser builds its own
        self.proposal = SceneParser(cfg, B, device=dev, mask_threshold=self.mask_threshold)
        self.n_bands = int(H.lib().air_canvas_unroll_bands(B, int(Hi)))
        with torch.cuda.device(dev):
            self.res_parts = torch.zeros((Rn, self.n_bands, B), device=dev)
            self.residual_energy = torch.zeros((Rn, B), device=dev)
        self._search = prune.SubsetSearchRounds(H, eng, Rn, T, self.proposals, B, self.n_bands)
        self._search.alias(self)
        # the read-out of the last round's first T rows (what the parsers keep)
        self._ro = ReadOut(H, eng, T, B, cfg.n_appearance, cfg.img_size, self.n_bands, self.mask_threshold)
        self._ro.alias(self)
        self.residual = self.proposal.engine.obs.view(B, Hi, Wi)
        self._H = H
        self._rebuild()
        eng.synchronize()
        self.proposal.engine.synchronize()

    def rows(self):
        """the provider protocol (stage.py): the compacted rows; presence_prob and the images are the start parse's"""
        return compacted_rows(self, self._start["presence_prob"], self._start["obs"])

    # ---- the launches behind the provider's own call -------------------------------------------------------------------------
    def _build_plan(self):
        H, eng, par, st, ieng, search = self._H, self.engine, self.parser, self._start, self.proposal.engine, self._search
        cfg = eng.cfg
        check_arguments(cfg, self.proposals, self.rounds)
        L, p, size = H.lib(), H._p, ctypes.c_size_t
        T, B, A, P = self.T, self.R, int(cfg.n_appearance), self.proposals
        (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
        self.segments = []                                         # per round: {name: launch list}, the names of SEGMENTS
        for r in range(self.rounds):
            (what, where, glimpse, score), presence, n_in, src_in = search.current(r, st, par.score, par.presence, None)
            seg = {
                "residual": [
                    (L.air_propose_residual,
                     (p(glimpse), p(where), presence, n_in, p(st["obs"]), float(cfg.output_multiplier), self.clamp_hi, T, B, Hi, Wi, hc,
                      wc, self.n_bands, p(ieng.obs), p(self.res_parts[r])), "air_propose_residual"),
                    (L.air_sum_leading, (p(self.res_parts[r]), p(self.residual_energy[r]), self.n_bands, size(B)), "air_sum_leading")],
                "forward": list(ieng._plan_fwd),
                "pool": [
                    (L.air_propose_pool,
                     (p(what), p(where), p(glimpse), p(score), presence, n_in, src_in, p(ieng.what), p(ieng.where),
                      p(ieng.gd.out[-1]), p(ieng.step_w), p(eng.prior_dev), r, T, P, B, A, hc * wc, *search.pool_out(r)),
                     "air_propose_pool")]}
            seg.update(search.search(r, st["obs"], self.normalize_steps_prior))
            self.segments.append(seg)
        self.readout = search.readout(self._ro, st["presence_prob"], st["obs"])
        self._plan = [e for seg in self.segments for name in SEGMENTS for e in seg[name]] + self.readout
        self._built_on = ieng._plan_fwd

    def _plan_is_current(self):
        """... and the proposal engine has not rebuilt its forward plan, a part of this one"""
        return super()._plan_is_current() and self.proposal.engine._plan_fwd is self._built_on

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call behind the bound provider's own (`parser` holds that provider's launch_count()); the
        per-round entries are counted over all rounds"""
        n = self.rounds
        return {"parser": self.parser.launch_count(), "propose_residual": n, "residual_sum": n,
                "forward": n * len(self.proposal.engine._plan_fwd), "propose_pool": n, "prune_score": n, "prune_select": n,
                "propose_source": n, "parse_objects": 1, "prune_relabel": 1, "parse_render": 1, "rec_sum": 1}

    # ---- parameters: the bound provider's AND the proposal engine's ----------------------------------------------------------------
    def load_from(self, train_engine):
        self.parser.load_from(train_engine)
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

    def capture(self):
        """every launch behind the provider's own call -- all rounds and the read-out -- as ONE hipGraph (the provider's graphs are its
        own: `parser.capture()`)"""
        self.proposal.engine.synchronize()
        super().capture()

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
        eng = self.engine
        self._refresh_plan()
        base = self.parser.parse(obs, *args, **kwargs)
        self.check_parse(base, "proposer")
        self._order_engines(True)
        eng._replay_or_run(self._graph, self._plan)
        self._order_engines(False)
        eng.wait_for_engine()
        return self._result(base)

    def _result(self, base):
        out = self._search.result(base, self.parser, self._ro, "objects_proposed_kept")
        out.update({"residual": self.residual, "residual_energy": self.residual_energy})
        return out
