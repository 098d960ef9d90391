"""What the post-parse stages share: the provider protocol, the read-out of a table of objects, the life cycle of a bound stage.

A PROVIDER is anything whose `parse()` leaves a parse in device buffers a later stage reads in place.  It says what it is:

  KIND     "scene" (parse.SceneParser), "particle" (particle_parse.ParticleParser), "refiner" (refine.ParseRefiner), "subset"
           (prune.ParsePruner, propose.ParseProposer, temporal.TemporalProposer), "tiled" (tile.TiledSceneParser), "completed"
           (trajectory.CompletedFrames);
  rows()   the buffers its `parse()` returns the parse in: what [T, R, A], where [T, R, 4], glimpse [T, R, G], presence_prob [T, R]
           (the START parse's; None where there is none), obs (its R-row images), where_loc (the rows that centre a shift prior given
           without `loc`; None: there are none to read in place), gather_loc (True: particle 0's where_loc rows are to be gathered from
           the K * R-row engine before every call), and compacted (True: the rows are a leading-ones chain the provider compacted
           itself, its count is `num_objects` and it has no presence chain of the inference network to read);
  and the public read-out attributes num_objects, count_prob, presence, score, boxes, offsets, obj_*, reconstruction, rec, owner, area,
  next to T, R, engine, mask_threshold, launch_count(), load_from / load_parameters / set_global_step / update_config / synchronize.

A stage states the kinds it binds to (`ACCEPTS`) and refuses the rest (`BoundStage.bind`); nothing looks at a provider's other
attributes to find out what it is.  `ReadOut` owns the read-out buffers and writes the argument order of air_parse_objects,
air_prune_relabel / air_tile_relabel, air_parse_render and air_sum_leading once.  `BoundStage` is the life cycle of an object that binds
to a provider and runs a launch list behind that provider's own call: the plan and what it holds by value of the engine's configuration,
the captured graph, the forwarding of parameters and run-time switches.  Which stages stand behind a parse, and how the built stacks
are cached, is stacks.py's.  Pure Python; torch is imported where it is needed.
"""
import ctypes

from .launch import destroy_graphs

KINDS = ("scene", "particle", "refiner", "subset", "tiled", "completed")
ROW_KEYS = ("what", "where", "glimpse", "presence_prob")
READOUT_KEYS = ("num_objects", "count_prob", "presence", "score", "boxes", "offsets", "obj_image", "obj_step", "obj_box", "obj_score",
                "obj_where", "obj_what", "reconstruction", "rec", "owner", "area")


def engine_rows(eng):
    """rows() of a provider that leaves its parse in its own engine's buffers (parse.SceneParser)"""
    return {"what": eng.what, "where": eng.where, "glimpse": eng.gd.out[-1], "presence_prob": eng.presence_prob, "obs": eng.obs,
            "where_loc": eng.where_loc, "gather_loc": False, "compacted": False}


def compacted_rows(owner, presence_prob, obs):
    """rows() of a provider that keeps compacted rows of its own under what / where / glimpse"""
    return {"what": owner.what, "where": owner.where, "glimpse": owner.glimpse, "presence_prob": presence_prob, "obs": obs,
            "where_loc": None, "gather_loc": False, "compacted": True}


def prior_arguments(cfg):
    """(what_loc, what_scale, scale_loc, scale_scale, shift_loc, shift_scale) as the kernels take them: NaN for a shift prior given
    without `loc` (the convention of air_iw_logweight)"""
    shift_loc = cfg.where_shift_prior[0]
    return (float(cfg.what_prior[0]), float(cfg.what_prior[1]), float(cfg.where_scale_prior[0]), float(cfg.where_scale_prior[1]),
            float("nan") if shift_loc is None else float(shift_loc), float(cfg.where_shift_prior[1]))


class ReadOut:
    """The read-out of a table of T rows by N columns (appearance size A, image H x W, the reconstruction term in n_bands row bands):
    its buffers, and the launches that fill them.  `with_rec=False`: a table without images to compare with (no rec_parts / rec)."""

    def __init__(self, H, engine, T, N, A, img_size, n_bands, mask_threshold, keep_layers=False, with_rec=True):
        import torch
        self._H, self.engine = H, engine
        self.T, self.N, self.A, self.img_size, self.n_bands = int(T), int(N), int(A), (int(img_size[0]), int(img_size[1])), int(n_bands)
        self.mask_threshold = float(mask_threshold)
        T, N, A, (Hi, Wi), dev = self.T, self.N, self.A, self.img_size, engine.device
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.num_objects, self.count_prob = z((N,), torch.int32), z((N,))
            self.presence, self.score, self.boxes = z((T, N)), z((T, N)), z((T, N, 4))
            self.offsets = z((N + 1,), torch.int32)
            self.obj_image, self.obj_step = z((T * N,), torch.int32), z((T * N,), torch.int32)
            self.obj_box, self.obj_score = z((T * N, 4)), z((T * N,))
            self.obj_where, self.obj_what = z((T * N, 4)), z((T * N, A))
            self.reconstruction = z((N, Hi, Wi))
            self.rec_parts, self.rec = (z((self.n_bands, N)), z((N,))) if with_rec else (None, None)
            self.owner = z((N, Hi, Wi), torch.int8)
            self.area = z((T, N), torch.int32)
            self.layers = z((T, N, Hi, Wi)) if keep_layers else None

    def tensors(self, **renamed):
        """{name: buffer} of everything the read-out owns, `renamed` mapping a name to the one the owner knows it by"""
        return {renamed.get(k, k): getattr(self, k) for k in READOUT_KEYS + ("rec_parts",) if getattr(self, k) is not None}

    def alias(self, owner, **renamed):
        """the owner exposes the buffers as attributes of its own: what other stages, the tools and the tests read"""
        for k, v in self.tensors(**renamed).items():
            setattr(owner, k, v)

    # ---- the launches ---------------------------------------------------------------------------------------------------------
    def objects(self, presence_prob, counts, where, what):
        """air_parse_objects: presence_prob None = there is no count posterior (count_prob stays 0), counts None = the mode"""
        L, p = self._H.lib(), self._H._p
        return (L.air_parse_objects,
                (p(presence_prob), p(counts), p(where), p(what), self.T, self.N, self.A, *self.img_size, p(self.num_objects),
                 p(self.count_prob), p(self.presence), p(self.score), p(self.boxes), p(self.offsets), p(self.obj_image),
                 p(self.obj_step), p(self.obj_box), p(self.obj_score), p(self.obj_where), p(self.obj_what)), "air_parse_objects")

    def relabel(self, entry, score_src, ids):
        """air_prune_relabel / air_tile_relabel (`entry`): score / obj_score from score_src, obj_step from ids"""
        L, p = self._H.lib(), self._H._p
        return (getattr(L, entry), (p(score_src), p(ids), p(self.num_objects), p(self.offsets), self.T, self.N, p(self.score),
                                    p(self.obj_score), p(self.obj_step)), entry)

    def render(self, glimpse, where, obs):
        """air_parse_render with the engine's output_multiplier / output_std as they are NOW (the plan holds them by value)"""
        L, p, cfg = self._H.lib(), self._H._p, self.engine.cfg
        (hc, wc) = cfg.crop_size
        return (L.air_parse_render,
                (p(glimpse), p(where), p(self.presence), p(obs), float(cfg.output_multiplier), float(cfg.output_std),
                 self.mask_threshold, self.T, self.N, *self.img_size, hc, wc, self.n_bands, p(self.reconstruction), p(self.rec_parts),
                 p(self.owner), p(self.area), p(self.layers)), "air_parse_render")

    def rec_sum(self):
        L, p = self._H.lib(), self._H._p
        return (L.air_sum_leading, (p(self.rec_parts), p(self.rec), self.n_bands, ctypes.c_size_t(self.N)), "air_sum_leading")

    def tail(self, glimpse, where, obs):
        return [self.render(glimpse, where, obs), self.rec_sum()]

    def result(self, glimpse):
        """the keys every parse result has from the read-out, and `glimpse` [T, N, G] viewed as crops"""
        out = {k: getattr(self, k) for k in READOUT_KEYS}
        out["glimpse"] = glimpse.view(self.T, self.N, *self.engine.cfg.crop_size)
        return out


class BoundStage:
    """An object that binds to a provider (`self._bound`: what parameters and switches are forwarded to) and runs `self._plan`, captured
    as ONE hipGraph by `capture()`, behind that provider's own call on the provider's engine stream.  A subclass sets ACCEPTS, REFUSALS
    (kind -> the ValueError text), KEY_FIELDS (the configuration fields its plan holds by value) and `_build_plan()`."""
    ACCEPTS = ()
    REFUSALS = {}
    KEY_FIELDS = ()
    _graph = None

    @classmethod
    def bind(cls, provider):
        """the provider's rows(), or the refusal of a kind this stage does not bind to"""
        kind = getattr(provider, "KIND", None)
        if kind not in cls.ACCEPTS:
            raise ValueError(cls.REFUSALS.get(kind) or "%s binds to a provider of kind %s, got %r (%s)"
                             % (cls.__name__, " / ".join(cls.ACCEPTS), kind, type(provider).__name__))
        return provider.rows()

    # ---- the plan -------------------------------------------------------------------------------------------------------------
    def _plan_key(self):
        """what of the engine's configuration the launch list holds by value"""
        cfg = self.engine.cfg
        return tuple(getattr(cfg, k) for k in self.KEY_FIELDS)

    def _plan_is_current(self):
        return self._plan_key() == self._built_for

    def _rebuild(self):
        self._build_plan()
        self._built_for = self._plan_key()

    def _refresh_plan(self):
        """rebuild (and re-capture, if a graph was held) when a switch of the provider's engine moved without this object being told:
        the provider is also used on its own, and its `update_config` does not know what is bound to it"""
        if self._plan_is_current():
            return False
        had = self._graph is not None
        self.release_graphs()
        self._rebuild()
        if had:
            self.capture()
        return True

    # ---- graphs ---------------------------------------------------------------------------------------------------------------
    def _score_entries(self):
        """further {"plan", "graph"} entries captured and released with the stage's own graph"""
        return ()

    def capture(self):
        """every launch behind the provider's own call as ONE hipGraph (the provider's graphs are its own: its `capture()`)"""
        self.release_graphs()
        self.engine.synchronize()
        self._graph = self.engine._capture_plans([self._plan])
        for entry in self._score_entries():
            entry["graph"] = self.engine._capture_plans([entry["plan"]])

    def release_graphs(self):
        entries = list(self._score_entries())
        destroy_graphs([self._graph] + [e["graph"] for e in entries])
        self._graph = None
        for e in entries:
            e["graph"] = None

    # ---- parameters and switches: the bound provider's --------------------------------------------------------------------------
    def load_from(self, train_engine):
        """the bound provider takes another engine's parameters, step counter and run-time switches (its own `load_from`)"""
        self._bound.load_from(train_engine)
        self._refresh_plan()

    def load_parameters(self, named):
        self._bound.load_parameters(named)

    def set_global_step(self, step: int):
        self._bound.set_global_step(step)

    def update_config(self, **changes) -> bool:
        """run-time switches of the bound provider's engine (AIREngine.KNOBS): the provider re-captures its graphs, this object rebuilds
        its launch list and re-captures when a value it holds changed.  A held graph may be destroyed: the engine's stream is drained
        first"""
        if self._graph is not None:
            self.engine.synchronize()
        changed = self._bound.update_config(**changes)
        return self._refresh_plan() or changed

    def synchronize(self):
        self.engine.synchronize()

    # ---- running ----------------------------------------------------------------------------------------------------------------
    def run_segments(self, *names):
        """issue the named segments eagerly, in the order given, on the engine's stream (tests and probes run the pieces this way);
        a stage whose segments are per round takes the round first"""
        eng, segments = self.engine, self.segments
        if isinstance(segments, list):
            segments, names = segments[names[0]], names[1:]
        eng.wait_for_caller()
        for name in names:
            eng._run(segments[name], eng._sp())
        eng.wait_for_engine()

    def gather_where_loc(self):
        """the one launch in front of the graph behind a provider with `gather_loc` and a shift prior given without `loc`: particle 0's
        where_loc rows into `self.where_loc` by a strided device copy on the engine stream (the library has no strided-gather entry;
        the particles of an image share where_loc)"""
        import torch
        eng = self.engine
        if self._start["gather_loc"] and eng.cfg.where_shift_prior[0] is None:
            with torch.cuda.stream(eng.stream):
                self.where_loc.copy_(eng.where_loc.view(self.T, self.R, -1, 4)[:, :, 0], non_blocking=True)

    def check_parse(self, base, who):
        """the bound provider's result must come from the buffers `self._start` (its rows()) and its read-out attributes name"""
        par, st = self._bound, self._start
        self.check_same_buffers(base, dict({k: st[k] for k in ROW_KEYS}, presence=par.presence, score=par.score,
                                           num_objects=par.num_objects), who)

    @staticmethod
    def check_same_buffers(base, expected, who, bound="parser"):
        """`base` (the bound provider's result) must hold, under every key of `expected`, the very buffer the plan was built on"""
        for k, buf in expected.items():
            if base[k].data_ptr() != buf.data_ptr():
                raise RuntimeError("the bound %s returned %r from another buffer than the %s was built on" % (bound, k, who))

    def check_render(self, entry, refusal):
        """air_parse_render stages the rows' bordered glimpses and the axis tables of a band in LDS: refuse here, by name, a table it
        declines (status -5; its first launch on the still empty rows decides)"""
        from . import _lib
        fn, args, name = entry
        st = fn(*args, self.engine._sp())
        if st == -5:
            raise ValueError(refusal)
        _lib.check(st, name)
