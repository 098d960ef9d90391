"""Recovering objects a frame's parse missed from its neighbour frames: the proposals of propose.py, taken from frames f - 1 and f + 1.

track.py gives identities to what each frame's parse found, but every frame is parsed alone: an object the inference network missed in
frame f can only be coasted over.  The strongest evidence a sequence offers is the same object, already inferred with `what`, `where`
and a decoded glimpse, one frame earlier and one frame later.  This module puts those rows into the exact subset search of prune.py and
lets the generative model decide -- by the arg-max of log p(x_f, z_S) -- whether they belong in frame f.  No network is evaluated.

Layout.  The provider has R = S F rows, sequence-major: row r = s F + f (the tracker's layout).  One round, on the `current rows` of
ALL frames at once (round 0: the provider's parse; later: the first T rows the previous round left), for row r in this order
(air_temporal_pool; include/air_hip.h states the same):

  1. boxes       the box of any row is evaluation.attention_box(where, W, H) in fp32, the bits of air_parse_objects' boxes;
  2. candidates  q = 0 .. 2T-1: q < T is slot q of frame f - 1, otherwise slot q - T of frame f + 1, read from this round's INPUT rows
                 of the same sequence (Jacobi); never across a sequence boundary;
  3. states      ABSENT (no such frame, direction="past" and q >= T, or slot >= the neighbour's count), NONFINITE (a where, score or
                 what value is not finite), KNOWN (IoU(box_q, box_j) > iou_novel, strictly, for a current object j: air_score_match's
                 float64 box IoU);
  4. the walk    the remaining candidates by score descending (equal: the lower q): DUPLICATE of the first already TAKEN d with
                 IoU(box_q, box_d) > iou_novel, otherwise TAKEN while fewer than P are, else FULL;
  5. partner     of the i-th taken d: the first DUPLICATE of d in walk order from the OTHER side; with interpolate and a partner c
                 the pool's where row is (float)(0.5 * ((double) where_d + (double) where_c)) -- tx, ty are linear in position, so for
                 linear motion this is the object's place in frame f -- otherwise where_d's bits; what, glimpse, score are d's bits;
  6. pool        C = T + P <= 6 rows: the T current rows, then the taken candidates (bit copies), then filler rows (what = NaN, where =
                 (1, 0, 1, 0), glimpse = 0, score = 0, source -1: every subset containing one has a NaN joint, which the selection never
                 takes); pool_presence = the current chain, pool_source = where every row came from (a taken candidate q of round k:
                 T + k * 2T + q), pool_prior = the count table followed by zeros, so the selected count stays <= T;
  7. search      air_prune_score / air_prune_select unchanged, with T := C, every row a candidate, obs = the frame itself;
  8. source      air_propose_source: source_out[j] = pool_source[kept_step[j]].

Between rounds the first T compacted rows, the counts and source_out of all frames are the next round's input: with rounds = 2 an
object can travel two frames.  After the last round the proposer's read-out runs (air_parse_objects in its given-counts form with the
START parse's presence_prob, air_prune_relabel, air_parse_render, air_sum_leading).  Guarantees (propose.py's, for the same reasons):
the per-frame objective never decreases over rounds; objective_start of round r + 1 is objective of round r bit for bit; a frame whose
every round keeps its start mask returns the provider's parse bit for bit; the count never exceeds T.  With F = 1 no candidate exists
and a round is the subset search of prune.ParsePruner("all") over the frame's own rows (the search may still drop or switch on rows of
the provider's parse, as ParseProposer's does): behind a provider whose parse is a fixed point of that search -- a ParsePruner("all"),
a ParseProposer -- every frame keeps its start mask and F = 1 returns the provider's parse bit for bit.  Behind a pruner or proposer
kept_step / obj_step index that provider's compacted rows.

`TemporalProposer` owns no engine: it binds to a parse.SceneParser, refine.ParseRefiner, prune.ParsePruner or propose.ParseProposer at
R = S F rows, runs that provider's own `parse()` and then, on the same engine stream, its launch list -- all rounds and the read-out
are ONE hipGraph after `capture()`; the provider's buffers are only read.  It exposes the provider surface ParseProposer has, so
track.SequenceTracker and score.ParseScorer bind to it as to every other provider.  A particle_parse.ParticleParser and a
tile.TiledSceneParser (its rows are scene slots, up to 32) are refused.

Out of scope: re-refining accepted proposals, motion models beyond the two-neighbour midpoint, neighbours further than one frame per
round, tiled and particle providers.  The defaults iou_novel = 0.3, proposals = 1, rounds = 1, interpolate = True are provisional:
UNMEASURED on a trained model (profiles/temporal.txt says what was measured).  `reference_pool` restates the kernel in numpy float64;
the search is prune.reference_score / prune.reference_select.
"""
import math
from typing import Dict

from . import prune
from .engine_config import EngineConfig
from .stage import BoundStage, ReadOut, compacted_rows
from .tile import box_iou, scene_boxes

MAX_POOL = prune.MAX_STEPS                                         # air_prune_score is instantiated up to 6 rows
SEGMENTS = ("pool", "score", "select", "source")
ABSENT, TAKEN, KNOWN, DUPLICATE, FULL, NONFINITE = range(6)
STATES = ("absent", "taken", "known", "duplicate", "full", "nonfinite")
DIRECTIONS = {"past": 0, "both": 1}
DEFAULTS = dict(proposals=1, rounds=1, iou_novel=0.3, direction="both", interpolate=True)
FILLER_WHERE = (1.0, 0.0, 1.0, 0.0)


def max_proposals(max_steps: int) -> int:
    """the most proposal rows a round can add: the 2T candidates, and a pool of at most 6 rows"""
    return min(2 * int(max_steps), MAX_POOL - int(max_steps))


def check_arguments(cfg: EngineConfig, n_frames, n_rows=None, proposals: int = 1, rounds: int = 1, iou_novel: float = 0.3):
    """Refuse what cannot be proposed this way (pure host code: importable and callable without a GPU).  Returns (T, F, S) with
    S = None when `n_rows` is not given."""
    prune.check_arguments(cfg, "all")
    T = int(cfg.max_steps)
    if isinstance(proposals, bool) or int(proposals) != proposals or not 1 <= int(proposals) <= max_proposals(T):
        raise ValueError("proposals: between 1 and min(2 * max_steps, %d - max_steps) = %d neighbour rows per round (the candidate pool "
                         "holds max_steps + proposals rows and the subset search stops at %d rows), got %r"
                         % (MAX_POOL, max_proposals(T), MAX_POOL, proposals))
    if isinstance(rounds, bool) or int(rounds) != rounds or int(rounds) < 1:
        raise ValueError("rounds must be an integer >= 1, got %r" % (rounds,))
    iou = float(iou_novel)
    if not (math.isfinite(iou) and 0.0 <= iou <= 1.0):
        raise ValueError("iou_novel must be a number within [0, 1], got %r" % (iou_novel,))
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or int(n_frames) < 1:
        raise ValueError("n_frames must be an integer >= 1, got %r" % (n_frames,))
    F, S = int(n_frames), None
    if n_rows is not None:
        if int(n_rows) < 1 or int(n_rows) % F:
            raise ValueError("the provider's %d rows are no multiple of %d frames" % (int(n_rows), F))
        S = int(n_rows) // F
    if cfg.where_shift_prior[0] is None:
        raise ValueError("temporal proposals need where_shift_prior with a `loc`: a shift prior centred on where_loc needs the where_loc "
                         "row of every pool row, and neither a neighbour's row nor the compaction carries them")
    return T, F, S


def reference_pool(what, where, glimpse, score, n, prior, n_frames, img_size, proposals=1, iou_novel=0.3, both_sides=True,
                   interpolate=True, round=0, source_in=None):
    """air_temporal_pool restated in numpy float64, with the same operation order.  Current rows what [T, R, A], where [T, R, 4],
    glimpse [T, R, G], score [T, R] (fp32), n [R] (clipped to 0..T), prior [T+1], R = S * n_frames, img_size = (H, W).  Returns what /
    where / glimpse / score [C, R, .] float32, presence [C, R] float32, source [C, R] int32, prior [C+1] float64, cand_state [R, 2T]
    int8, taken [R] int32, partner [P, R] int32, and boxes [T, R, 4] float32 (the rows' boxes)."""
    import numpy as np
    what, where, glimpse, score = (np.asarray(a, np.float32) for a in (what, where, glimpse, score))
    T, R, A = what.shape
    G = glimpse.shape[2]
    F, P = int(n_frames), int(proposals)
    if F < 1 or R % F:
        raise ValueError("%d rows are no multiple of %d frames" % (R, F))
    if not 1 <= T <= MAX_POOL or not 1 <= P <= max_proposals(T):
        raise ValueError("T within 1..%d and proposals within 1..min(2T, %d - T), got T = %d, proposals = %d" % (MAX_POOL, MAX_POOL, T, P))
    C, thr = T + P, float(iou_novel)
    n = np.clip(np.asarray(n).astype(np.int64), 0, T)
    boxes = scene_boxes(where, img_size)
    out = {"what": np.empty((C, R, A), np.float32), "where": np.empty((C, R, 4), np.float32),
           "glimpse": np.empty((C, R, G), np.float32), "score": np.empty((C, R), np.float32),
           "presence": (np.arange(C)[:, None] < n[None, :]).astype(np.float32), "source": np.empty((C, R), np.int32),
           "prior": np.concatenate([np.asarray(prior, np.float64)[:T + 1], np.zeros(P)]),
           "cand_state": np.zeros((R, 2 * T), np.int8), "taken": np.zeros(R, np.int32), "partner": np.full((P, R), -1, np.int32),
           "boxes": boxes}
    for k in ("what", "where", "glimpse", "score"):
        out[k][:T] = locals()[k]
    out["source"][:T] = np.arange(T)[:, None] if source_in is None else np.asarray(source_in)[:T]
    out["what"][T:], out["where"][T:], out["glimpse"][T:], out["score"][T:], out["source"][T:] = np.nan, FILLER_WHERE, 0.0, 0.0, -1
    for r in range(R):
        f = r % F
        state = np.zeros(2 * T, np.int64)
        open_q = []
        row_of = lambda q: (q, r - 1) if q < T else (q - T, r + 1)
        for q in range(2 * T):
            slot, nr = row_of(q)
            if (q < T and f == 0) or (q >= T and (f == F - 1 or not both_sides)) or slot >= n[nr]:
                continue                                           # ABSENT
            if not (np.isfinite(where[slot, nr]).all() and np.isfinite(score[slot, nr]) and np.isfinite(what[slot, nr]).all()):
                state[q] = NONFINITE
            elif any(box_iou(boxes[slot, nr], boxes[j, r]) > thr for j in range(n[r])):
                state[q] = KNOWN
            else:
                open_q.append(q)
        open_q.sort(key=lambda q: (-float(score[row_of(q)]), q))
        taken, mate = [], []
        for q in open_q:
            dup = next((i for i, d in enumerate(taken) if box_iou(boxes[row_of(q)], boxes[row_of(d)]) > thr), None)
            if dup is not None:
                state[q] = DUPLICATE
                if (q >= T) != (taken[dup] >= T) and mate[dup] < 0:
                    mate[dup] = q
            elif len(taken) < P:
                state[q] = TAKEN
                taken.append(q)
                mate.append(-1)
            else:
                state[q] = FULL
        out["cand_state"][r], out["taken"][r] = state, len(taken)
        for i, d in enumerate(taken):
            src = row_of(d)
            out["partner"][i, r] = mate[i]
            out["what"][T + i, r], out["glimpse"][T + i, r], out["score"][T + i, r] = what[src], glimpse[src], score[src]
            out["where"][T + i, r] = where[src]
            if interpolate and mate[i] >= 0:
                out["where"][T + i, r] = (0.5 * (where[src].astype(np.float64) + where[row_of(mate[i])].astype(np.float64))
                                          ).astype(np.float32)
            out["source"][T + i, r] = T + int(round) * 2 * T + d
    return out


class TemporalProposer(BoundStage):
    KIND = "subset"
    ACCEPTS = ("scene", "refiner", "subset")
    REFUSALS = {
        "particle": "a ParticleParser is out of scope for temporal proposals (its rows are particles of an image, not images): "
                    "bind a SceneParser, ParseRefiner, ParsePruner or ParseProposer",
        "tiled": "a TiledSceneParser is out of scope for temporal proposals (its rows are scene slots, up to 32, and the subset "
                 "search stops at %d rows): bind a SceneParser, ParseRefiner, ParsePruner or ParseProposer" % MAX_POOL}
    KEY_FIELDS = prune.ParsePruner.KEY_FIELDS

    def __init__(self, provider, n_frames, proposals: int = DEFAULTS["proposals"], rounds: int = DEFAULTS["rounds"],
                 iou_novel: float = DEFAULTS["iou_novel"], direction: str = DEFAULTS["direction"],
                 interpolate: bool = DEFAULTS["interpolate"], normalize_steps_prior: bool = True):
        rows = self.bind(provider)
        cfg = provider.engine.cfg
        if direction not in DIRECTIONS:
            raise ValueError('direction must be "past" or "both", got %r' % (direction,))
        T, F, S = check_arguments(cfg, n_frames, provider.R, proposals, rounds, iou_novel)
        import torch
        from . import hip as H
        self.parser, self.engine = provider, provider.engine
        self._bound = provider
        self.proposals, self.rounds, self.iou_novel = int(proposals), int(rounds), float(iou_novel)
        self.direction, self.interpolate = direction, bool(interpolate)
        self.normalize_steps_prior = bool(normalize_steps_prior)
        self.T, self.R, self.S, self.F = int(provider.T), int(provider.R), S, F
        self.C = self.T + self.proposals
        self.mask_threshold = provider.mask_threshold
        eng, dev = self.engine, self.engine.device
        T, B, P, Rn = self.T, self.R, self.proposals, self.rounds
        self.n_bands = int(H.lib().air_canvas_unroll_bands(B, int(cfg.img_size[0])))
        # what round 0 reads: the provider's rows and per-step score, and its presence chain -- or, behind compacted rows, its counts
        comp = rows["compacted"]
        self._start = dict(rows, score=provider.score, presence=None if comp else provider.presence,
                           counts=provider.num_objects if comp else None)
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.cand_state, self.proposals_taken = z((Rn, B, 2 * T), torch.int8), z((Rn, B), torch.int32)
            self.partner = z((Rn, P, B), torch.int32)
        self._search = prune.SubsetSearchRounds(H, eng, Rn, T, P, B, self.n_bands)
        self._search.alias(self)
        # the read-out of the last round's first T rows (what the parsers keep)
        self._ro = ReadOut(H, eng, T, B, cfg.n_appearance, cfg.img_size, self.n_bands, self.mask_threshold)
        self._ro.alias(self)
        self._H = H
        self._rebuild()
        eng.synchronize()

    def rows(self):
        """the provider protocol (stage.py): the compacted rows; presence_prob and the images are the start parse's"""
        return compacted_rows(self, self._start["presence_prob"], self._start["obs"])

    # ---- the launches behind the provider's own call -------------------------------------------------------------------------
    def _build_plan(self):
        H, eng, st, search = self._H, self.engine, self._start, self._search
        cfg = eng.cfg
        check_arguments(cfg, self.F, self.R, self.proposals, self.rounds, self.iou_novel)
        L, p = H.lib(), H._p
        T, A, P = self.T, int(cfg.n_appearance), self.proposals
        (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
        both, mid = DIRECTIONS[self.direction], 1 if self.interpolate else 0
        self.segments = []                                         # per round: {name: launch list}, the names of SEGMENTS
        for r in range(self.rounds):
            (what, where, glimpse, score), presence, n_in, src_in = search.current(r, st, st["score"], st["presence"], st["counts"])
            seg = {"pool": [(L.air_temporal_pool,
                             (p(what), p(where), p(glimpse), p(score), presence, n_in, src_in, p(eng.prior_dev), r, T, P, self.S,
                              self.F, A, hc * wc, Hi, Wi, self.iou_novel, both, mid, *search.pool_out(r), p(self.cand_state[r]),
                              p(self.proposals_taken[r]), p(self.partner[r])), "air_temporal_pool")]}
            seg.update(search.search(r, st["obs"], self.normalize_steps_prior))
            self.segments.append(seg)
        self.readout = search.readout(self._ro, st["presence_prob"], st["obs"])
        self._plan = [e for seg in self.segments for name in SEGMENTS for e in seg[name]] + self.readout

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call behind the bound provider's own (`parser` holds that provider's launch_count()); the
        per-round entries are counted over all rounds"""
        n = self.rounds
        return {"parser": self.parser.launch_count(), "temporal_pool": n, "prune_score": n, "prune_select": n, "propose_source": n,
                "parse_objects": 1, "prune_relabel": 1, "parse_render": 1, "rec_sum": 1}

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def parse(self, obs, *args, **kwargs):
        """obs: the frames as the provider's R = S F rows, row s F + f (further arguments go to the provider's `parse()` unchanged),
        then the rounds and the read-out.  Returns device tensors that the NEXT call overwrites: every key of the provider's result and
        of ParseProposer.parse with the same meaning -- num_objects, count_prob, presence, score, boxes, what, where, glimpse, the
        object table, reconstruction, rec, owner, area describe the parse after the last round (row j is pool row kept_step[j]);
        presence_prob, num_steps_posterior and a provider's other read-outs are the provider's; objective / objective_start [R]
        float64 are J after the last round / of the start parse; objective_subsets [R, 2^C], best_mask [R] and evidence [C, R] are the
        LAST round's, over its pool; objective_rounds [rounds + 1, R]; num_objects_start [R];
        kept_step [T, R] int32 is source_out: a value < T is a start step (row kept_step of the provider's parse), otherwise
        kept_step - T = round * 2T + q names candidate q of that round -- and
          cand_state [rounds, R, 2T] int8 (STATES), proposals_taken [rounds, R] int32, partner [rounds, P, R] int32,
          proposal_what / proposal_where / proposal_glimpse / proposal_score [rounds, P, R, .] (the pool's proposal rows, filler
          rows included), objects_temporal_kept [R] int32 (objects of the result that came from a neighbour frame);
        behind a ParseRefiner also refine_objective, refine_objective_start; behind a ParsePruner or ParseProposer that provider's
        objective / objective_start as provider_objective / provider_objective_start.  Same stream contract as the parsers."""
        eng = self.engine
        self._refresh_plan()
        base = self.parser.parse(obs, *args, **kwargs)
        self.check_parse(base, "proposer")
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        return self._result(base)

    def _result(self, base):
        out = self._search.result(base, self.parser, self._ro, "objects_temporal_kept")
        out.update({"cand_state": self.cand_state, "proposals_taken": self.proposals_taken, "partner": self.partner})
        return out
