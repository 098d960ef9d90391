"""AIRonMNIST -- AIR for the multi-MNIST dataset with the constructor of the reference
(attend_infer_repeat/mnist_model.py:10-44): n_appearance=50, LSTM(256) transition, output_std=.3, stock modules.

Because this is the standard architecture, `train_step` runs through the fused hipGraph-captured engine
(engine.AIREngine) instead of autograd; the module tree shares its parameters with the engine's flat buffer, so
cell-by-cell calls and `forward()` always see the trained weights.
"""
from functools import partial

import torch

from .engine import AIREngine, EngineConfig
from .model import AIRModel
from .modules import BaselineMLP, Decoder, Encoder, StepsPredictor, StochasticTransformParam
from . import stacks
from .rnn import LSTM


class AIRonMNIST(AIRModel):
    """Implements AIR for the MNIST dataset"""

    def __init__(self, obs, nums, glimpse_size=(20, 20),
                 inpt_encoder_hidden=[256] * 2,
                 glimpse_encoder_hidden=[256] * 2,
                 glimpse_decoder_hidden=[252] * 2,
                 transform_estimator_hidden=[256] * 2,
                 steps_pred_hidden=[50] * 1,
                 baseline_hidden=[256, 128] * 1,
                 transform_var_bias=-2.,
                 step_bias=0.,
                 *args, **kwargs):
        self.transform_var_bias = torch.tensor(float(transform_var_bias))     # non-trainable variables,
        self.step_bias = torch.tensor(float(step_bias))                       # mnist_model.py:24-26
        self.baseline = BaselineMLP(baseline_hidden)
        # (extension, default None: the reference's objective) the default of train_step's `iw_samples`
        self.iw_samples = kwargs.pop("iw_samples", None)
        self._iw_objective_default = kwargs.pop("iw_objective", None)          # ... and of its `iw_objective`
        self._hyper = dict(inpt_encoder_hidden=tuple(inpt_encoder_hidden),
                           glimpse_encoder_hidden=tuple(glimpse_encoder_hidden),
                           glimpse_decoder_hidden=tuple(glimpse_decoder_hidden),
                           transform_estimator_hidden=tuple(transform_estimator_hidden),
                           steps_pred_hidden=tuple(steps_pred_hidden), baseline_hidden=tuple(baseline_hidden))
        super(AIRonMNIST, self).__init__(
            *args,
            obs=obs,
            nums=nums,
            glimpse_size=glimpse_size,
            n_appearance=50,
            transition=LSTM(256),
            input_encoder=partial(Encoder, inpt_encoder_hidden),
            glimpse_encoder=partial(Encoder, glimpse_encoder_hidden),
            glimpse_decoder=partial(Decoder, glimpse_decoder_hidden),
            transform_estimator=partial(StochasticTransformParam, transform_estimator_hidden,
                                        scale_bias=self.transform_var_bias),
            steps_predictor=partial(StepsPredictor, steps_pred_hidden, self.step_bias),
            output_std=.3,
            **kwargs
        )

    # ---- name map between the module tree and the engine's flat parameter buffer -------------------------------------
    def _named_module_params(self):
        c = self.cell
        out = {}

        def mlp(prefix, m):
            for i, layer in enumerate(m.layers):
                out[f"{prefix}/{i}/w"], out[f"{prefix}/{i}/b"] = layer.w, layer.b

        mlp("input_encoder", c._input_encoder.mlp)
        out["lstm/w_gates"], out["lstm/b_gates"] = c._transition.w_gates, c._transition.b_gates
        out["lstm/h0"], out["lstm/c0"] = c._transition.h0, c._transition.c0
        mlp("transform", c._transform_estimator.mlp)
        mlp("steps", c._steps_predictor.mlp)
        mlp("glimpse_encoder", c._glimpse_encoder.mlp)
        out["what/w"], out["what/b"] = c._what_distrib.w, c._what_distrib.b
        mlp("glimpse_decoder", c._glimpse_decoder.mlp)
        bm = getattr(self, "baseline_module", None)
        if bm is not None and all(l.w is not None for l in bm.mlp.layers):   # built lazily by the first _reinforce call
            mlp("baseline", bm.mlp)
        return out

    def _engine_eligible(self, use_engine, l2_weight, what_prior, where_scale_prior, where_shift_prior, num_steps_prior,
                         decay_rate):
        """The fused engine takes the reference script's configuration (scripts/multi_mnist.py:24-94) and, since round 5, the rest
        of train_step's plain arguments (model.py:261-353): l2_weight, decay_rate (EMA-normalised importance weights), a weighted
        num-steps prior, a where-shift prior without `loc`, the RMSProp keyword set (decay / momentum / epsilon / centered), a
        what / where prior left at None (model.py:174, 187: the term is not added) and a non-analytic num-steps prior (sampled step
        weights, the prior inside the importance weight: model.py:157-163, 339-340).
        Continuous steps (discrete_steps=False, cell.py:150-151: the presence is the probability itself and carries a gradient
        through the canvas write) run on the engine too.  What still trains through the generic autograd path over the same kernels:
        a custom optimizer CLASS and a non-MLP baseline.  num_steps_prior=None is an error in the reference too (model.py:157 reads
        its `analytic`)."""
        nsp = num_steps_prior
        has = lambda p, *keys: p is not None and all(k in p for k in keys)
        if not use_engine:
            return False
        if getattr(self, "_iw_samples", None) is not None:   # the K-particle objective trains through the generic autograd path
            return False
        if getattr(self, "_custom_optimizer", None) is not None:
            return False
        if nsp is None:
            return False
        if what_prior is not None and not has(what_prior, 'loc', 'scale'):
            return False
        if where_scale_prior is not None and where_shift_prior is not None and not (
                has(where_scale_prior, 'loc', 'scale') and has(where_shift_prior, 'scale')):
            return False
        if decay_rate is not None and not self.use_reinforce:
            return False
        if self.use_reinforce:
            bm = getattr(self, "baseline_module", None)
            if not isinstance(bm, BaselineMLP) or any(l.w is None for l in bm.mlp.layers):
                return False
        return True

    def engine_config(self, learning_rate, num_steps_prior, what_prior, where_scale_prior, where_shift_prior, l2_weight=0.,
                      decay_rate=None):
        nsp = num_steps_prior
        rms = getattr(self, "_rms_kwargs", None) or dict(decay=0.9, momentum=0.9, epsilon=1e-10, centered=True)
        has_where = where_scale_prior is not None and where_shift_prior is not None
        return EngineConfig(
            img_size=tuple(self.img_size), crop_size=tuple(self.glimpse_size), n_appearance=self.n_appearance,
            n_hidden=256, max_steps=self.max_steps,
            transform_var_bias=float(self.transform_var_bias), step_bias=float(self.step_bias),
            output_multiplier=float(self.output_multiplier), output_std=float(self.output_std),
            explore_eps=None if self.explore_eps is None else float(self.explore_eps),
            what_prior=None if what_prior is None else (what_prior.loc, what_prior.scale),
            where_scale_prior=None if not has_where else (where_scale_prior.loc, where_scale_prior.scale),
            where_shift_prior=None if not has_where else (where_shift_prior.loc if 'loc' in where_shift_prior else None,
                                                          where_shift_prior.scale),
            nsp_analytic=bool(getattr(nsp, 'analytic', True)), discrete_steps=bool(self.discrete_steps),
            nsp_anneal=getattr(nsp, 'anneal', None), nsp_init=nsp.init, nsp_final=getattr(nsp, 'final', nsp.init),
            nsp_steps_div=getattr(nsp, 'steps_div', 1.), nsp_steps=getattr(nsp, 'steps', 1.),
            nsp_hold_init=getattr(nsp, 'hold_init', 0.),
            use_prior=self.use_prior, use_reinforce=self.use_reinforce, learning_rate=float(learning_rate),
            guard_eps=float(getattr(self, 'guard_degenerate', 0.0)),
            l2_weight=float(l2_weight or 0.), decay_rate=None if decay_rate is None else float(decay_rate),
            nsp_weight=float(getattr(nsp, 'weight', 1.)), rms_decay=float(rms["decay"]), rms_momentum=float(rms["momentum"]),
            rms_eps=float(rms["epsilon"]), rms_centered=bool(rms["centered"]), **self._hyper)

    def train_step(self, learning_rate, l2_weight=0., what_prior=None, where_scale_prior=None,
                   where_shift_prior=None, num_steps_prior=None, use_prior=True, use_reinforce=True, baseline=None,
                   decay_rate=None, optimizer=None, opt_kwargs=None, use_engine=True, capture_graph=True,
                   mfma_dtype="f32", iw_samples=None, iw_objective=None):
        """model.py:261-376 on the fused engine.  Extras over the reference signature: `use_engine` / `capture_graph`, and
        `mfma_dtype` ("f32" exact fp32 MFMA, "bf16" = bf16-rounded operands with fp32 accumulate in every dense product).
        `iw_samples=K` (None: the constructor's, itself None by default): the K-particle importance-weighted objective of
        AIRModel.train_step, on the generic autograd path -- the engine, its plans and its graphs are not built.
        `iw_objective` (None: the constructor's): its estimator, "vimco" (the default) or "rws" (reweighted wake-sleep)."""
        if iw_samples is None:
            iw_samples = self.iw_samples
        if iw_objective is None:
            iw_objective = self._iw_objective_default
        fn, gs = super(AIRonMNIST, self).train_step(learning_rate, l2_weight, what_prior, where_scale_prior,
                                                    where_shift_prior, num_steps_prior, use_prior, use_reinforce,
                                                    baseline, decay_rate, optimizer, opt_kwargs, iw_samples=iw_samples,
                                                    iw_objective=iw_objective)
        if not self._engine_eligible(use_engine, l2_weight, what_prior, where_scale_prior, where_shift_prior,
                                     num_steps_prior, decay_rate):
            return fn, gs
        self._hyper["mfma_dtype"] = mfma_dtype
        cfg = self.engine_config(learning_rate, num_steps_prior, what_prior, where_scale_prior, where_shift_prior, l2_weight,
                                 decay_rate)
        eng = AIREngine(cfg, self.batch_size, device=self.obs.device)
        named = self._named_module_params()
        eng.load_parameters({k: v.detach() for k, v in named.items()})
        eng.synchronize()
        for k, p in named.items():                           # share storage: modules now view the engine's flat buffer
            p.data = eng.params[k]
        eng.set_obs(self.obs)
        if capture_graph:
            eng.capture()
        self._engine = eng

        state = {"lr": None}

        def train_step_fn(obs=None, nums=None, refresh=True):
            """One fused update (fresh noise, forward, backward, both RMSProp updates) as a hipGraph replay.
            refresh=False skips re-exposing the engine buffers as model attributes (a device sync + a handful of torch
            ops per call): use it in tight training loops and call `air.refresh()` / `air.evaluate(...)` when needed."""
            if obs is not None:
                self.obs = obs
            if nums is not None:
                self.nums = nums
            lr = float(self.learning_rate)
            if lr != state["lr"]:
                eng.set_learning_rate(lr); state["lr"] = lr
            self._sync_engine_switches()
            eng.train_step(obs)
            self.global_step += 1
            if refresh:
                self._refresh_from_engine()
            return self.global_step

        self._train_step = train_step_fn
        return self._train_step, self.global_step

    def _sync_engine_switches(self):
        """The reference's non-trainable variables (use_prior / toggle_prior, explore_eps, step_bias, transform_var_bias,
        output_multiplier: model.py:58,71,307-308, mnist_model.py:24-26) are plain attributes here; whatever they hold NOW is
        what the next engine launch uses (AIREngine.update_config re-captures when one of them changed)."""
        eng = self._engine
        if eng is not None:
            eng.update_config(use_prior=bool(self.use_prior),
                              explore_eps=None if self.explore_eps is None else float(self.explore_eps),
                              step_bias=float(self.step_bias), transform_var_bias=float(self.transform_var_bias),
                              output_multiplier=float(self.output_multiplier))

    def forward(self, obs=None, nums=None, noise=None):
        """Generic cell-by-cell unroll (model.py:66-104).  Once the engine owns the parameters the module tree aliases its
        flat buffer, so this torch-stream pass is ordered after the engine's pending updates, and the engine's next launch
        after this pass."""
        eng = getattr(self, "_engine", None)
        if eng is not None:
            eng.wait_for_engine()
        out = super(AIRonMNIST, self).forward(obs, nums, noise)
        if eng is not None:
            eng.wait_for_caller()
        return out

    def evaluate(self, obs=None, nums=None, noise=None):
        """Engine-backed evaluation pass (fresh noise, no update); falls back to the generic path without an engine."""
        if self._engine is None:
            return super(AIRonMNIST, self).evaluate(obs, nums, noise)
        if obs is not None:
            self.obs = obs
        if nums is not None:
            self.nums = nums
        self._sync_engine_switches()
        self._engine.forward(self.obs, sample_noise=True)
        self._refresh_from_engine()
        return self

    def iw_evaluator(self, particles=16):
        """the ImportanceEvaluator behind evaluate_iw (built and captured on first use, rebuilt when `particles` changes)"""
        eng = stacks.require_engine(self, "evaluate_iw")
        from .iw_eval import ImportanceEvaluator
        return stacks.slot(self, "_iw_evaluator", lambda ev: ev.K == int(particles) and ev.B == eng.B and ev.engine.device == eng.device,
                           lambda: ImportanceEvaluator(eng.cfg, eng.B, int(particles), device=eng.device))

    def evaluate_iw(self, obs=None, nums=None, particles=16):
        """K-particle importance-weighted evaluation on the device (iw_eval.ImportanceEvaluator: its own engine at
        particles * batch_size rows, its own noise stream -- the training engine's parameters are read, nothing of it is
        written).  Sets iw_bound / iw_elbo / iw_ess (batch means), iw_bound_per_sample [B], iw_num_steps_posterior [B, T+1]
        (self-normalised posterior over the object count) and, with `nums`, iw_num_step_accuracy (its argmax against the truth)."""
        ev = self.iw_evaluator(particles)
        eng = self._engine
        if obs is not None:
            self.obs = obs
        if nums is not None:
            self.nums = nums
        self._sync_engine_switches()
        ev.load_from(eng)                                    # every time: the weights move
        gt = None if self.nums is None else self.nums.sum(0).reshape(-1)
        out = ev.evaluate(self.obs, gt)                      # (the caller's stream is ordered after it: the reads below are safe)
        self.iw_bound_per_sample = out["iw_bound"]
        self.iw_bound, self.iw_elbo, self.iw_ess = out["iw_bound"].mean(), out["elbo"].mean(), out["ess"].mean()
        self.iw_num_steps_posterior = out["num_steps_posterior"]
        if gt is not None:
            self.iw_num_step_accuracy = (out["num_steps_posterior"].argmax(-1) == gt.to(torch.int64)).float().mean()
        return self

    def scene_sampler(self, n_scenes=None):
        """the SceneSampler behind sample_scenes (built and captured on first use, rebuilt when the size or the device changes;
        n_scenes=None: the size it has, the batch size on first use)"""
        eng = stacks.require_engine(self, "sample_scenes")
        from .generate import SceneSampler
        s = getattr(self, "_scene_sampler", None)
        n = int(n_scenes) if n_scenes is not None else (s.R if s is not None else eng.B)
        return stacks.slot(self, "_scene_sampler", lambda s: s.R == n and s.device == eng.device,
                           lambda: SceneSampler(eng.cfg, n, device=eng.device))

    def sample_scenes(self, n_scenes=None, num_objects=None, count_probs=None):
        """Scenes from the generative model on the device (generate.SceneSampler: the trained decoder is copied, nothing of the
        training engine is written).  count_probs: None = the model's own count prior at the current step (collapsed onto n = 0
        once annealed -- see SceneSampler), 'uniform', or max_steps + 1 weights; num_objects: condition on these counts instead.
        Sets generated_obs / generated_mean [N, H, W], generated_num_objects [N], generated_what [T, N, A], generated_where
        [T, N, 4], generated_presence [T, N] and generated_glimpse [T, N, h, w]; the next call overwrites them."""
        s = self.scene_sampler(n_scenes)
        self._sync_engine_switches()
        s.load_from(self._engine)                            # every time: the weights move
        s.set_count_probs(count_probs)
        out = s.sample(num_objects=num_objects)              # (the caller's stream is ordered after it)
        self.generated_obs, self.generated_mean, self.generated_num_objects = out["obs"], out["mean"], out["num_objects"]
        self.generated_what, self.generated_where, self.generated_presence = out["what"], out["where"], out["presence"]
        self.generated_glimpse = out["glimpse"]
        return self

    def scene_parser(self, batch_size=None):
        """the SceneParser behind parse (built and captured on first use, rebuilt when the size or the device changes;
        batch_size=None: the size it has, the batch size on first use)"""
        eng = stacks.require_engine(self, "parse")
        from .parse import SceneParser
        s = getattr(self, "_scene_parser", None)
        n = int(batch_size) if batch_size is not None else (s.R if s is not None else eng.B)
        return stacks.slot(self, "_scene_parser", lambda s: s.R == n and s.engine.device == eng.device,
                           lambda: SceneParser(eng.cfg, n, device=eng.device))

    def particle_parser(self, batch_size=None, particles=16, select="joint"):
        """the ParticleParser behind parse(particles=K) (built and captured on first use, rebuilt when the size, K, the criterion or
        the device changes; batch_size=None: the size it has, the batch size on first use)"""
        eng = stacks.require_engine(self, "parse")
        from .particle_parse import ParticleParser
        s = getattr(self, "_particle_parser", None)
        n = int(batch_size) if batch_size is not None else (s.B if s is not None else eng.B)
        return stacks.slot(self, "_particle_parser",
                           lambda s: s.B == n and s.K == int(particles) and s.select == select and s.engine.device == eng.device,
                           lambda: ParticleParser(eng.cfg, n, int(particles), select=select, device=eng.device))

    def _scorer(self, name, parser, max_gt_objects, thresholds):
        """the score.ParseScorer held under `self.<name>` (built and captured on first use, rebuilt when the parser, the number of
        ground-truth slots or the thresholds change)"""
        from .score import DEFAULT_THRESHOLDS, ParseScorer
        th = tuple(float(t) for t in (DEFAULT_THRESHOLDS if thresholds is None else thresholds))
        return stacks.slot(self, name, lambda s: s.parser is parser and s.G == int(max_gt_objects) and s.thresholds_host == th,
                           lambda: ParseScorer(parser, max_gt_objects, th))

    MAX_PARSE_REFINERS = MAX_PARSE_PRUNERS = MAX_PARSE_PROPOSERS = 4
    MAX_TILED_PARSERS = MAX_TRACKERS = MAX_TEMPORAL_PROPOSERS = 2

    def _cache(self, name):
        """the stacks.BoundedCache `self._<name>` of at most MAX_<NAME> entries (the limit is read when used)"""
        return self.__dict__.setdefault("_" + name, stacks.BoundedCache(lambda: getattr(self, "MAX_" + name.upper())))

    def _parser_for(self, particles, select, refine=None, refine_lr=None, prune=None, propose=None):
        spec = stacks.stack_spec(refine, refine_lr, prune, propose, who="parse")
        n = self.obs.shape[0]
        parser = self.scene_parser(n) if particles is None else self.particle_parser(n, particles, select)
        if spec.refine is not None:
            parser = self.parse_refiner(parser, spec.refine, spec.lr)
        if spec.propose is not None:
            return self.parse_proposer(parser, spec.propose)
        return parser if spec.prune is None else self.parse_pruner(parser, spec.prune)

    def _parse_stage(self, name, provider, key, spec, refiners=()):
        """The stage `spec` asks for behind `provider` in the cache `name` of `parse`: built and captured on first use; an entry found
        under `key` but bound to another provider is released and rebuilt; dropped first is what is bound to neither the current scene
        parser, the current particle parser nor one of `refiners`."""
        alive = [getattr(self, "_scene_parser", None), getattr(self, "_particle_parser", None)] + list(refiners)
        cache = self._cache(name)
        cache.drop(lambda r: not any(r.parser is a for a in alive))
        return cache.get(key, lambda: stacks.captured(stacks.build_stack(provider, spec)[-1]), lambda r: r.parser is provider)

    def parse_refiner(self, parser, steps, lr=None):
        """the ParseRefiner behind parse(refine=N): one per (batch, particles, select, N, lr), bound to that parser (built and captured
        on first use; dropped when its parser was rebuilt, and the least recently used one when more than MAX_PARSE_REFINERS are
        alive -- a scorer still bound to a dropped one keeps working, its refiner then launches eagerly)"""
        spec = stacks.stack_spec(refine=steps, refine_lr=lr)
        key = (parser.R, getattr(parser, "K", None), getattr(parser, "select", None), spec.refine, spec.lr)
        return self._parse_stage("parse_refiners", parser, key, spec)

    def parse_pruner(self, provider, candidates="present"):
        """the ParsePruner behind parse(prune=...): one per (provider, candidates), bound to that scene parser, particle parser or
        refiner (built and captured on first use; dropped when its provider was rebuilt or dropped, and the least recently used one
        when more than MAX_PARSE_PRUNERS are alive -- a scorer still bound to a dropped one keeps working, its pruner then launches
        eagerly)"""
        return self._parse_stage("parse_pruners", provider, (id(provider), candidates), stacks.stack_spec(prune=candidates),
                                 self._cache("parse_refiners").values())

    def parse_proposer(self, provider, propose=1):
        """the ParseProposer behind parse(propose=...): one per (provider, proposals, rounds), bound to that scene parser, particle
        parser or refiner (built and captured on first use; dropped when its provider was rebuilt or dropped, and the least recently
        used one when more than MAX_PARSE_PROPOSERS are alive -- a scorer still bound to a dropped one keeps working, its proposer
        then launches eagerly).  propose: P, or (P, rounds)."""
        spec = stacks.stack_spec(propose=propose)
        return self._parse_stage("parse_proposers", provider, (id(provider),) + spec.propose, spec, self._cache("parse_refiners").values())

    def parse(self, obs=None, num_objects=None, particles=None, select="joint", refine=None, refine_lr=None, prune=None, propose=None):
        """Scene parse on the device.  particles=None: the deterministic parse (parse.SceneParser: its own engine at the mode of the
        inference network); particles=K: K posterior particles per image and the best one under `select` ("joint": the largest
        log p(x, z), "weight": the largest importance weight) kept (particle_parse.ParticleParser: its own engine at K * batch
        rows, its own noise stream).  The training engine's parameters are read, nothing of it is written.  obs=None: the model's
        current batch.  Returns the parser's dict of device tensors (SceneParser.parse lists them: num_objects, count_prob,
        presence, score, boxes, what, where, the object table behind offsets, reconstruction, rec, owner, area; ParticleParser.parse
        adds best_particle, the weights, the spread of `where`); the next call overwrites them.  num_objects (counts to use instead
        of the model's) goes with the deterministic parse only.  refine=N: N gradient-ascent iterations on log p(x, z) behind that
        parse (refine.ParseRefiner; refine_lr = (lr_what, lr_where), None: refine.DEFAULT_LR); the result then describes the refined
        parse and adds objective, objective_start, best_iter, objective_trace, grad_what, grad_where.  refine=None: the paths above,
        untouched.  prune="present" | "all": behind whichever of the paths above, the exact arg-max of log p(x, z_S) over the subsets
        S of the computed steps (prune.ParsePruner; max_steps <= 6) -- "present" can only remove objects of the parse, "all" may also
        switch on a step the presence chain left out; the result then describes the selected subset, compacted, and adds objective,
        objective_start (float64), objective_subsets, best_mask, kept_step, evidence, num_objects_start.  prune=None: the paths
        above, untouched.  propose=P | (P, rounds): behind whichever of the paths above (not together with prune: the search over
        the pool contains prune="all"), `rounds` rounds of P proposals from the residual image and the exact subset search over the
        pool of max_steps + P <= 6 rows (propose.ParseProposer); the result has the pruner's keys -- kept_step now names start steps
        (< max_steps) and proposals (max_steps + round * P + j) -- and adds objective_rounds, residual, residual_energy,
        proposal_what / _where / _glimpse / _score, objects_proposed_kept.  propose=None: the paths above, untouched."""
        if particles is not None and num_objects is not None:
            raise ValueError("parse: num_objects together with particles is not supported (conditioning the sampled chain on a "
                             "count is out of scope); pass one of them")
        if obs is not None:
            self.obs = obs
        s = self._parser_for(particles, select, refine, refine_lr, prune, propose)
        self._sync_engine_switches()
        s.load_from(self._engine)                            # every time: the weights move
        # (the caller's stream is ordered after it)
        self.parsed = s.parse(self.obs, num_objects) if particles is None else s.parse(self.obs)
        return self.parsed

    def parse_scorer(self, max_gt_objects, thresholds=None, particles=None, select="joint", refine=None, refine_lr=None, prune=None,
                     propose=None):
        """the ParseScorer behind score_parse, bound to the parser of the current batch size that parse(particles=..., select=...)
        uses (built and captured on first use, rebuilt when the parser, the number of ground-truth slots or the thresholds change);
        refine=N binds it to that parse's refiner instead, so the refined parse is what gets scored; prune=... to that parse's pruner,
        propose=... to that parse's proposer"""
        return self._scorer("_parse_scorer", self._parser_for(particles, select, refine, refine_lr, prune, propose), max_gt_objects,
                            thresholds)

    def score_parse(self, obs, gt_instances, gt_boxes, gt_count=None, thresholds=None, accumulate=True, particles=None,
                    select="joint", refine=None, refine_lr=None, prune=None, propose=None):
        """Parse `obs` (AIRonMNIST.parse, with `particles` / `select` as there), then score the parse against the ground truth on the device (score.ParseScorer.score lists
        the arguments and the returned device tensors).  gt_count=None: the number of rows of gt_boxes with width > 0.  The sums
        accumulate in `parse_scorer(...)`: its reset() starts a validation set, its summary() reads the figures back once."""
        self.parse(obs, particles=particles, select=select, refine=refine, refine_lr=refine_lr, prune=prune, propose=propose)
        s = self.parse_scorer(torch.as_tensor(gt_boxes).shape[1], thresholds, particles, select, refine, refine_lr, prune, propose)
        self.parse_scores = s.score(gt_instances, gt_boxes, gt_count, accumulate=accumulate)
        return self.parse_scores

    def _own_stack(self, rows, spec, n_frames=None):
        """a provider stack of its own at `rows` rows on the training engine's device: a SceneParser and behind it what `spec` asks
        for (stacks.build_stack), so that the parsers of `parse` and `self.obs` are never touched"""
        from .parse import SceneParser
        return stacks.build_stack(SceneParser(self._engine.cfg, rows, device=self._engine.device), spec, n_frames)

    def tiled_parser(self, n_scenes, scene_size, stride=None, iou_merge=0.5, refine=None, refine_lr=None, prune=None, propose=None):
        """the tile.TiledSceneParser behind parse_tiled: one per (n_scenes, scene_size, stride, iou_merge, refine, refine_lr, prune,
        propose), over a provider stack of its own at n_scenes * windows rows -- a SceneParser, behind it the refiner / pruner /
        proposer asked for -- so the parsers of `parse` and `self.obs` are never touched.  Built and captured on first use; the
        least recently used one is dropped, with its stack, when more than MAX_TILED_PARSERS are alive (each owns an engine)."""
        eng = stacks.require_engine(self, "parse_tiled")
        spec = stacks.stack_spec(refine, refine_lr, prune, propose, who="parse_tiled")
        from . import tile
        (Hs, Ws), (sy, sx), (ny, nx) = tile.check_arguments(eng.cfg, scene_size, stride, iou_merge, int(n_scenes))

        def build():
            stack = self._own_stack(int(n_scenes) * ny * nx, spec)
            return stacks.captured(stack + [tile.TiledSceneParser(stack[-1], (Hs, Ws), (sy, sx), iou_merge)])
        key = (int(n_scenes), (Hs, Ws), (sy, sx), float(iou_merge), spec, str(eng.device))
        return self._cache("tiled_parsers").get(key, build)[-1]

    def parse_tiled(self, scenes, stride=None, iou_merge=0.5, refine=None, refine_lr=None, prune=None, propose=None):
        """Parse scenes [S, Hs, Ws] LARGER than the model's canvas on the device: overlapping windows of the canvas's size at `stride`
        (None: half the canvas), each parsed as `parse(refine=, prune=, propose=)` would parse it, and the windows' objects merged
        into one parse per scene (tile.TiledSceneParser.parse lists the returned device tensors; the next call overwrites them).
        The training engine's parameters are read, nothing of it is written; `self.obs` and the parsers of `parse` are not touched."""
        scenes = torch.as_tensor(scenes)
        if scenes.dim() != 3:
            raise ValueError("parse_tiled: scenes [S, Hs, Ws], got shape %s" % (tuple(scenes.shape),))
        s = self.tiled_parser(scenes.shape[0], tuple(scenes.shape[1:]), stride, iou_merge, refine, refine_lr, prune, propose)
        self._sync_engine_switches()
        s.load_from(self._engine)                            # every time: the weights move
        self.parsed_tiled = s.parse(scenes)
        return self.parsed_tiled

    def score_parse_tiled(self, scenes, gt_instances, gt_boxes, gt_count=None, thresholds=None, accumulate=True, stride=None,
                          iou_merge=0.5, refine=None, refine_lr=None, prune=None, propose=None):
        """parse_tiled, then score the scene parses against scene-level ground truth on the device (score.ParseScorer.score lists the
        arguments and the returned tensors; gt_instances [S, Hs, Ws], gt_boxes [S, G, 4] with G <= 8).  The sums accumulate in the
        scorer this returns alongside: (scores, scorer)."""
        self.parse_tiled(scenes, stride, iou_merge, refine, refine_lr, prune, propose)
        scenes = torch.as_tensor(scenes)
        parser = self.tiled_parser(scenes.shape[0], tuple(scenes.shape[1:]), stride, iou_merge, refine, refine_lr, prune, propose)
        s = self._scorer("_tiled_scorer", parser, int(torch.as_tensor(gt_boxes).shape[1]), thresholds)
        self.parse_scores_tiled = s.score(gt_instances, gt_boxes, gt_count, accumulate=accumulate)
        return self.parse_scores_tiled, s

    def tracker(self, n_sequences, n_frames, **track_args):
        """the track.SequenceTracker behind `track` (`track_args` are `track`'s; `_tracker_entry` describes the cache; with smooth= the
        tracker of the stack that ends in the trajectory.TrajectorySmoother `trajectory_smoother` returns)"""
        return self._tracker_entry(self._track_key(n_sequences, n_frames, **track_args))[0]

    def trajectory_smoother(self, n_sequences, n_frames, smooth=True, **track_args):
        """the trajectory.TrajectorySmoother behind `track(smooth=)` and `predict_frames`: last in the cached stack of
        `tracker(..., smooth=smooth)`, bound to that stack's tracker (smoothed, gap-filled and extrapolated tracks; its defaults are
        provisional)"""
        if stacks.smooth_spec(smooth) is None:
            raise ValueError("trajectory_smoother: smooth must be True or a dict of TrajectorySmoother's arguments, got %r" % (smooth,))
        return self._tracker_entry(self._track_key(n_sequences, n_frames, smooth=smooth, **track_args))[1]

    def stitcher(self, n_sequences, n_frames, stitch=True, **track_args):
        """the track.TrackStitcher behind `track(stitch=)`: last in the cached stack of `tracker(..., stitch=stitch)`, bound to that
        stack's tracker (track fragments joined across occlusions longer than max_age; its defaults are provisional)"""
        if stacks.stitch_spec(stitch) is None:
            raise ValueError("stitcher: stitch must be True, a max_gap or a dict of TrackStitcher's arguments, got %r" % (stitch,))
        return self._tracker_entry(self._track_key(n_sequences, n_frames, stitch=stitch, **track_args))[1]

    def _track_key(self, n_sequences, n_frames, **track_args):
        """the stacks.TrackKey of the track family's arguments (stacks.track_key names them: an unknown one is its TypeError)"""
        return stacks.track_key(stacks.require_engine(self, "track"), n_sequences, n_frames, **track_args)

    def _track_stack(self, key):
        """the built and captured stack of a key of the track family (stacks.build_track_stack over a provider stack of its own at
        key.S * key.F rows), from the one cache of the family: the least recently used stack is dropped when more than MAX_TRACKERS
        are alive (each owns an engine)"""
        return self._cache("trackers").get(key, lambda: stacks.captured(
            stacks.build_track_stack(self._own_stack(key.S * key.F, key.stack, key.F), key)))

    def _tracker_entry(self, key):
        """(tracker, smoother | None) for the stacks.TrackKey `key` -- those of the cached stack whose track.SequenceTracker is behind
        `track`: one per (n_sequences, n_frames, iou_gate, appearance_weight, birth_score, max_age, refine, refine_lr, prune, propose,
        temporal, smooth, matching, motion, motion_gate), over a provider stack of its own at n_sequences * n_frames rows -- a SceneParser,
        behind it the refiner / pruner / proposer asked for and, last, with temporal=P | (P, rounds) a temporal.TemporalProposer
        (objects a frame's parse missed are proposed from its neighbour frames; its defaults are provisional) -- so the parsers of
        `parse` and `self.obs` are never touched.  temporal=None builds exactly the stack without it; so does smooth=None, and
        smooth=True | dict appends a trajectory.TrajectorySmoother bound to the tracker (part of the key).  None for one of the four
        association arguments: track.DEFAULTS (provisional).  matching=None | "greedy" is exactly the stack without the argument,
        "optimal" a tracker of its own with the optimal assignment (part of the key).  motion=None is exactly the stack without the
        argument; True | dict a tracker of its own that matches every track against its predicted box (track.py: MOTION; part of the
        key; with smooth=dict(...) motion=True takes the smoother's noise terms).  motion_gate=None is exactly the stack without the
        argument; True | a squared Mahalanobis distance a tracker of its own whose pairs are gated by the filter's covariance (track.py:
        THE GATE; part of the key; it needs motion).  stitch=None is exactly the stack without the argument; True | MAX_GAP | dict a
        stack of its own that ends in a track.TrackStitcher bound to the tracker (track.py: STITCHING; part of the key; refused with
        smooth=) -- the second member of the pair is then that stitcher.  Built and captured on first use; the least
        recently used one is dropped, with its stack, when more than MAX_TRACKERS are alive (each owns an engine)."""
        stack = self._track_stack(key)
        return (stack[-1], None) if key.smooth is None and key.stitch is None else (stack[-2], stack[-1])

    def noise_fitter(self, n_sequences, n_frames, shift_ratios=None, scale_ratios=None, velocity_ratio=None, **track_args):
        """the trajectory.TrajectoryNoiseFitter behind `fit_track_noise`: last in a cached stack of its own (stacks.fit_key, in the
        cache of `tracker`: it counts against MAX_TRACKERS) whose track.SequenceTracker it is bound to; `track_args` are `tracker`'s
        without smooth=.  Built and captured on first use."""
        return self._track_stack(stacks.fit_key(stacks.require_engine(self, "fit_track_noise"), n_sequences, n_frames, shift_ratios,
                                                scale_ratios, velocity_ratio, **track_args))[-1]

    def fit_track_noise(self, frames, shift_ratios=None, scale_ratios=None, velocity_ratio=None, zoom=0, accumulate=False, fit=True,
                        **track_args):
        """The trajectory smoother's noise terms by maximum likelihood from the tracks of frames [S, F, H, W] themselves -- no ground
        truth: the frames are tracked as `track(frames, **track_args)` tracks them, and the likelihood of every track's sightings
        under the constant-rate model is evaluated on the device on a grid of candidates (trajectory.TrajectoryNoiseFitter; None:
        half-decades of process noise / measurement noise from 1e-6 to 1e3 and the default velocity_var / measurement_noise).
        Returns trajectory.profile_fit's dict: process_noise, measurement_noise, velocity_var -- `track(frames, smooth={k: fit[k] for
        k in trajectory.FIT_KEYS})` takes them as they are, and so does the association itself: `fit = m.fit_track_noise(frames)`,
        `noise = {k: fit[k] for k in trajectory.FIT_KEYS}`, `m.track(frames, motion=noise, smooth=noise)`; `track_args` may carry
        motion= too (the tracks the terms are fitted to are then the motion-predicted ones) --, loglik, n_innovations, cell, on_edge,
        surface (and the grid they refer to).  zoom=k refines the grid k times around the best cell.  accumulate=True adds the frames to those of the calls before
        (`noise_fitter(...).reset()` starts over; zoom needs a single batch), fit=False only does that: no read-back, returns None.
        The training engine's parameters are read, nothing of it is written."""
        frames = torch.as_tensor(frames)
        if frames.dim() != 4:
            raise ValueError("fit_track_noise: frames [S, F, H, W], got shape %s" % (tuple(frames.shape),))
        f = self.noise_fitter(frames.shape[0], frames.shape[1], shift_ratios, scale_ratios, velocity_ratio, **track_args)
        self._sync_engine_switches()
        f.load_from(self._engine)                            # every time: the weights move
        self.tracked = f.track(frames, accumulate=bool(accumulate))
        self.track_noise_fit = f.fit(zoom) if fit else None
        return self.track_noise_fit

    def stream_tracker(self, n_sequences, chunk_frames, **stream_args):
        """the track.StreamTracker behind `track_stream`: identities over sequences of any length, fed in chunks of `chunk_frames`
        frames, the track table carried on the device between the calls (motion= and motion_gate= are refused: out of scope on a stream,
        track.MOTION_ON_A_STREAM).  One per (n_sequences, chunk_frames, the association
        arguments, refine, refine_lr, prune, propose, temporal, matching) under a key of its own (stacks.stream_key) in the cache of
        `tracker` -- it counts against MAX_TRACKERS with the one-shot trackers -- over a provider stack of its own at n_sequences *
        chunk_frames rows, so the parsers of `parse` and `self.obs` are never touched (a temporal proposer sees only its chunk).  Built
        and captured on first use.  Dropped from the cache, its stream is lost with it."""
        return self._track_stack(stacks.stream_key(stacks.require_engine(self, "track_stream"), n_sequences, chunk_frames,
                                                   **stream_args))[-1]

    def stream_smoother(self, n_sequences, chunk_frames, smooth=True, **stream_args):
        """the trajectory.StreamSmoother behind `track_stream(smooth=)`: fixed-lag smoothed, gap-filled rows `lag` frames late and a
        forecast per chunk.  smooth: True or dict(lag=, horizon=, process_noise=, measurement_noise=, velocity_var=) (lag None:
        max_age; the defaults are provisional); `stream_args` are `stream_tracker`'s.  Last in a cached stack of its own
        (stacks.stream_smoother_key) whose StreamTracker it is bound to: another stream than that of `stream_tracker` with the same
        arguments.  Built and captured on first use; counts against MAX_TRACKERS."""
        return self._track_stack(stacks.stream_smoother_key(stacks.require_engine(self, "track_stream"), n_sequences, chunk_frames, smooth,
                                                            **stream_args))[-1]

    def track_stream(self, frames, valid=None, reset=False, smooth=None, **stream_args):
        """The next chunk of a stream: frames [S, F, H, W] parsed as `track` parses them and associated with the tracks of the chunks
        before (track.StreamTracker.push lists the returned device tensors; prev_frame and the tracks' first / last are global frame
        indices).  valid [S]: the frames each sequence has in this chunk (None: all F).  reset=True restarts every sequence first, a
        list of sequence indices those (a slot reused for a new video).  `stream_args` are `stream_tracker`'s; the stream is that
        tracker's: the same arguments continue it.  The training engine's parameters are read, nothing of it is written; `self.obs`
        and the parsers of `parse` are not touched.  smooth=None is exactly the call without the argument; smooth=True | dict
        (`stream_smoother`) pushes through a trajectory.StreamSmoother -- a stream of its own -- and adds the emitted table sm_*,
        emit_frame, num_emitted and, with a horizon, fc_* and frames_pred (trajectory.StreamSmoother.result)."""
        frames = torch.as_tensor(frames)
        if frames.dim() != 4:
            raise ValueError("track_stream: frames [S, F, H, W], got shape %s" % (tuple(frames.shape),))
        if smooth is None:
            t = self.stream_tracker(frames.shape[0], frames.shape[1], **stream_args)
        else:
            t = self.stream_smoother(frames.shape[0], frames.shape[1], smooth, **stream_args)
        if reset is not False and reset is not None:
            t.reset(None if reset is True else reset)
        self._sync_engine_switches()
        t.load_from(self._engine)                            # every time: the weights move
        self.tracked_stream = t.push(frames, valid)
        return self.tracked_stream

    def temporal_proposer(self, n_sequences, n_frames, proposals=1, rounds=1, refine=None, refine_lr=None, prune=None, propose=None):
        """the temporal.TemporalProposer for callers who want the repaired per-frame parses without identities: one per (n_sequences,
        n_frames, proposals, rounds, refine, refine_lr, prune, propose), last in a provider stack of its own at n_sequences * n_frames
        rows (`tracker`'s).  Built and captured on first use; `load_from(self._engine)` before `parse(frames_as_rows)` is the
        caller's.  The least recently used one is dropped, with its stack, when more than MAX_TEMPORAL_PROPOSERS are alive."""
        eng = stacks.require_engine(self, "temporal_proposer")
        spec = stacks.stack_spec(refine, refine_lr, prune, propose, (proposals, rounds), who="temporal_proposer")
        from .temporal import check_arguments
        S, F = int(n_sequences), int(n_frames)
        if S < 1:
            raise ValueError("temporal_proposer: at least one sequence, got %r" % (n_sequences,))
        check_arguments(eng.cfg, F, S * F, *spec.temporal)
        return self._cache("temporal_proposers").get((S, F, spec, str(eng.device)),
                                                     lambda: stacks.captured(self._own_stack(S * F, spec, F)))[-1]

    def _track(self, frames, **track_args):
        """`track` with its arguments by name; returns the (tracker, smoother | stitcher | None) that ran"""
        frames = torch.as_tensor(frames)
        if frames.dim() != 4:
            raise ValueError("track: frames [S, F, H, W], got shape %s" % (tuple(frames.shape),))
        tracker, smoother = self._tracker_entry(self._track_key(frames.shape[0], frames.shape[1], **track_args))
        last = tracker if smoother is None else smoother
        self._sync_engine_switches()
        last.load_from(self._engine)                         # every time: the weights move
        self.tracked = last.track(frames)
        return tracker, smoother

    def track(self, frames, iou_gate=None, appearance_weight=None, birth_score=None, max_age=None, refine=None, refine_lr=None,
              prune=None, propose=None, temporal=None, smooth=None, matching=None, motion=None, motion_gate=None, stitch=None):
        """Parse the frames [S, F, H, W] of S sequences on the device, each frame as `parse(refine=, prune=, propose=)` would parse
        it -- with temporal=P | (P, rounds) followed by proposals from the neighbour frames (temporal.TemporalProposer) -- and give
        the objects identities over time (track.SequenceTracker.track lists the returned device tensors: the parse of
        the S * F frames, row s * F + f, and next to it track_id, obj_state, affinity, prev_frame, prev_slot, the per-track tables and
        track_owner; the next call overwrites them).  With smooth=True | dict(horizon=, process_noise=, measurement_noise=,
        velocity_var=) the tracks are then smoothed, gap-filled and extrapolated (trajectory.TrajectorySmoother.result lists the sm_
        and fc_ tensors and frames_pred that come on top); smooth=None is exactly the call without it.  matching="optimal": the
        optimal assignment of every frame instead of the greedy one (track.py states both rules).  motion=True | dict(process_noise=,
        measurement_noise=, velocity_var=): every track is matched against where a per-track Kalman filter PREDICTS it to be, not
        against its last box (track.py: MOTION; pred_where and pred_boxes come on top) -- an object missed for a frame or two while it
        moves keeps its id, two objects that cross keep theirs; motion=None is exactly the call without it.  The noise terms are the
        smoother's: `fit = m.fit_track_noise(frames)`, then `noise = {k: fit[k] for k in trajectory.FIT_KEYS}` and
        `m.track(frames, motion=noise, smooth=noise)` (motion=True with smooth=dict(...) takes the smoother's terms).
        motion_gate=True | D2 (with motion): the pairs are gated by their squared Mahalanobis distance from the filter's predicted
        state, D2 at most (True: track.MOTION_GATE_DEFAULT, provisional), and ranked by it instead of the IoU -- the fitted noise terms
        and the gate then concern one quantity; pred_d2 comes on top; motion_gate=None is exactly the call without it.
        stitch=True | MAX_GAP | dict(max_gap=, gate=, appearance_weight=, process_noise=, measurement_noise=, velocity_var=): a second
        pass joins a track that ended to one that began at most max_gap frames later when the first one's filter predicts the second
        one's first sighting and their `what` codes agree, the links by one optimal assignment (track.py: STITCHING; stitch_id, the
        stitch_ tables and stitch_owner come on top, the tracker's own outputs stay); stitch=None is exactly the call without it;
        together with smooth= it is refused.  The training
        engine's parameters are read, nothing of it is written; `self.obs` and the parsers of `parse` are not touched."""
        self._track(frames, iou_gate=iou_gate, appearance_weight=appearance_weight, birth_score=birth_score, max_age=max_age, refine=refine,
                    refine_lr=refine_lr, prune=prune, propose=propose, temporal=temporal, smooth=smooth, matching=matching, motion=motion,
                    motion_gate=motion_gate, stitch=stitch)
        return self.tracked

    def predict_frames(self, frames, horizon, smooth=True, **track_args):
        """`track(frames, smooth=...)` with a forecast horizon of `horizon` frames (1..16): returns (frames_pred [S, horizon, H, W],
        result) -- the frames F, F + 1, ... rendered from the tracks still live after the last frame, each at its extrapolated place
        with the decoded glimpse of its last sighting (no network evaluation); `result` is `track`'s dict.  `smooth` may carry the
        smoother's other arguments; its horizon is set from `horizon`."""
        spec = dict(stacks.smooth_spec(smooth) or stacks.smooth_spec(True))
        if isinstance(horizon, bool) or int(horizon) != horizon or int(horizon) < 1:
            raise ValueError("predict_frames: horizon must be an integer >= 1, got %r" % (horizon,))
        spec["horizon"] = int(horizon)
        out = self.track(frames, smooth=spec, **track_args)
        return out["frames_pred"], out

    def score_track(self, frames, gt_boxes, tau=0.5, accumulate=True, gt_instances=None, thresholds=None, iou_gate=None,
                    appearance_weight=None, birth_score=None, max_age=None, refine=None, refine_lr=None, prune=None, propose=None,
                    temporal=None, smooth=None, matching=None, identity=False, motion=None, motion_gate=None, hota=False, stitch=None,
                    mots=False):
        """`track`, then the identity metric of the tracks against gt_boxes [S, F, G, 4] (G <= 8; slot g is the same object in every
        frame of a sequence, width <= 0 = absent) on the device (track.SequenceTracker.score).  The sums accumulate in the tracker
        this returns alongside -- (scores, tracker): its summary() reads MOTA, MOTP, the identity switches and the mostly tracked /
        lost fractions back once, its reset() starts a validation set.  With gt_instances [S, F, H, W] (int8, -1 = background) the
        S * F frames are also scored as images by a score.ParseScorer bound to the same provider (per-frame detection figures next to
        the identity figures): scores["detection"] holds its tensors, `self.track_scorer` is that scorer.  With smooth= the COMPLETED
        table of the trajectory smoother is scored next to the raw one by the same kernel (TrajectorySmoother.score):
        scores["completed"] holds its tensors, `self.track_smoother` is the smoother, whose summary() / reset() are the completed
        table's -- the raw figures stay the tracker's.  matching= is `track`'s; identity=True adds the IDF1 counts (air_track_idf behind
        air_track_score: seq_idf, idf_overlap, totals_idf; the tracker's -- and the smoother's -- identity_summary() reads IDF1, IDP
        and IDR back).  motion= and motion_gate= are `track`'s.  hota=True also runs air_track_hota (track.SequenceTracker.hota): scores[
        "hota"] holds the tracker's tensors and totals (seq_hota_i, seq_hota_f, the tables, totals_hota_i / totals_hota_f), with smooth=
        scores["completed"]["hota"] the completed table's; hota_summary() of the tracker / the smoother reads HOTA, DetA, AssA and LocA
        back.  hota=False, the default: exactly the call without the argument.  stitch= is `track`'s: the STITCHED ids are scored
        (identity= and hota= included) by the track.TrackStitcher, which is then the stage returned alongside -- its summary() /
        identity_summary() / hota_summary() / reset() are the stitched table's, the tracker's totals are not touched.  mots=True (needs
        gt_instances) also scores the tracks as MASKS (track.SequenceTracker.mots: air_score_contingency of the owner map and the
        instance maps, then air_track_mots, with G slots as in gt_boxes): scores["mots"] holds the stage's tensors and totals
        (seq_mots_i, seq_mots_f, mots_match, mots_iou, cont, totals_mots_i / totals_mots_f), with smooth= scores["completed"]["mots"]
        the completed table's, with stitch= the stitched ids are scored; mots_summary() of the stage reads MOTSA, sMOTSA and MOTSP
        back.  mots=False, the default: exactly the call without the argument."""
        if mots and gt_instances is None:
            from .track import MOTS_NEEDS_INSTANCES
            raise ValueError(MOTS_NEEDS_INSTANCES)
        t, smoother = self._track(frames, iou_gate=iou_gate, appearance_weight=appearance_weight, birth_score=birth_score, max_age=max_age,
                                  refine=refine, refine_lr=refine_lr, prune=prune, propose=propose, temporal=temporal, smooth=smooth,
                                  matching=matching, motion=motion, motion_gate=motion_gate, stitch=stitch)
        if stacks.stitch_spec(stitch) is not None:                  # (never with smooth=: the key refuses it)
            t, smoother = smoother, None
        gb = torch.as_tensor(gt_boxes)
        scores = dict(t.score(gb, tau, accumulate, identity))
        if smoother is not None:
            self.track_smoother = smoother
            scores["completed"] = smoother.score(gb, tau, accumulate, identity)
        if hota:
            scores["hota"] = t.hota(gb, accumulate)
            if smoother is not None:
                scores["completed"] = dict(scores["completed"], hota=smoother.hota(gb, accumulate))
        if gt_instances is not None:
            G = int(gb.shape[-2])
            s = self._scorer("track_scorer", t.provider, G, thresholds)
            gi = torch.as_tensor(gt_instances)
            scores["detection"] = s.score(gi.reshape((t.R,) + tuple(gi.shape[-2:])), gb.reshape(t.R, G, 4), accumulate=accumulate)
            if mots:
                scores["mots"] = t.mots(gi, G, accumulate)
                if smoother is not None:
                    scores["completed"] = dict(scores["completed"], mots=smoother.mots(gi, G, accumulate))
        self.track_scores = scores
        return scores, t

    def refresh(self):
        """Re-expose the engine's current buffers under the reference's attribute names."""
        if self._engine is not None:
            self._refresh_from_engine()
        return self

    def _refresh_from_engine(self):
        """Expose the engine's buffers under the reference's attribute names (model.py:86-104,319-343)."""
        eng, T, B = self._engine, self.max_steps, self.batch_size
        o = eng.outputs()
        for k in ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale", "presence_prob", "presence",
                  "glimpse", "canvas", "final_canvas", "final_state", "rec_loss_per_sample", "rec_loss",
                  "kl_num_steps_per_sample", "kl_num_steps", "kl_what", "kl_where", "prior_step_weight",
                  "num_step_per_sample", "opt_loss", "reinforce_loss", "baseline_loss", "baseline"):
            if k == "kl_what" and eng.cfg.what_prior is None or k == "kl_where" and eng.cfg.where_scale_prior is None:
                continue                                   # model.py:174, 187: a prior left at None defines no such tensor
            if k in o:
                setattr(self, k, o[k])
        self.num_step = self.num_step_per_sample.mean()
        from .ops import Loss
        from .prior import NumStepsDistribution
        self.prior_loss = Loss(); self.prior_loss.add(o["prior_loss"], float(eng.cfg.nsp_weight) * o["kl_num_steps_per_sample"]
                                                      + o["kl_what_per_sample"] + o["kl_where_per_sample"])
        for k in ("l2_loss", "imp_weight_moving_mean", "imp_weight_moving_var"):
            if k in o:
                setattr(self, k, o[k])
        self.loss = Loss(); self.loss.add(o["loss"], o["rec_loss_per_sample"]
                                          + self.prior_weight * self.prior_loss.per_sample)
        if "baseline" in o:
            imp = o["rec_loss_per_sample"] if eng.cfg.nsp_analytic else o["rec_loss_per_sample"] + self.prior_loss.per_sample
            self.reinforce_imp_weight = imp                                                   # model.py:337-340
            self.importance_weight = imp[None, :] - o["baseline"]                             # [B,B] quirk, model.py:230
        self.num_steps_distrib = NumStepsDistribution(o["presence_prob"].reshape(T, B).t())
        self.steps_prior_success_prob = eng.steps_prior_success_prob(max(eng.global_step - 1, 0))
        if self.nums is not None:
            self.gt_num_steps = self.nums.sum(0).reshape(-1)
            self.num_step_accuracy = (self.gt_num_steps == self.num_step_per_sample).float().mean()
