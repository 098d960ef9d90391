"""Scene parsing with K posterior particles on the device: draw K explanations of every image from q(z | x), keep the best one.

    z_k ~ q(. | x),   k* = the smallest k attaining max_k s_k,   s_k = log w_k + log q(z_k | x) = log p(x, z_k)   ("joint")
                                                                  s_k = log w_k = log p(x, z_k) - log q(z_k | x)   ("weight")

`SceneParser` parses at the mode of the inference network.  AIR's posterior is discrete in the count and multimodal in `where`; a
model whose q is slightly off parses wrongly at the mode while one of its own samples explains the image well.  `ParticleParser`
owns an ordinary AIREngine at K * B rows (row r = b * K + k, as in iw_eval), runs that engine's own forward plan unchanged and
appends launches of libair_hip.so (include/air_hip.h describes them):

  air_iw_logweight     log w per row (unchanged);
  air_iw_logposterior  log q(z | x) per row;
  air_iw_reduce        the importance-weighted bound, the effective sample size, the self-normalised count posterior;
  air_particle_select  k* per image (NaN scores never win; all NaN: k* = 0 and degenerate = 1) and bit copies of the selected rows of
                       where / what / presence_prob / the decoder's raw glimpses into B-row buffers;
  air_particle_spread  per step and image the weighted mean / standard deviation of `where` over the particles that have the step, and
                       the weight share of those particles (a step no particle has: mean / std NaN, share exactly 0; a step exactly
                       one particle of non-zero weight has: its row, std exactly 0; an image whose weights are all -inf or hold a
                       +inf or a NaN: mean / std NaN (a NaN weight: at the steps that particle has) and the share of the class of the tail sums of air_iw_reduce's count posterior --
                       the reduce's convention, so `presence_iw` and `num_steps_posterior_iw` never disagree about such an image;
                       `degenerate` flags the all-NaN image, these outputs are not usable for it either way);
  air_parse_objects    given-counts form on the selected rows (count = n_{k*}; score = q(n > t), count_prob = q(n_{k*}));
  air_parse_render, air_sum_leading   as in parse.SceneParser, on the selected rows and a B-row copy of the images.

Ties are the common case, not a corner: the LSTM never sees the samples, so all particles of an image with n = 0 run the same
arithmetic on the same numbers -- their rows, log w and log q are bit-identical.  The rule "smallest k" makes the choice among
them (and every other exact tie) deterministic.  Noise, forward and all read-outs are one hipGraph per variant after `capture()`.
"""
import ctypes
from typing import Dict

from . import iw_eval
from .engine_config import EngineConfig
from .launch import destroy_graphs
from .stage import ReadOut

CRITERIA = {"weight": 0, "joint": 1}


def check_arguments(cfg: EngineConfig, batch_size: int, particles: int, select: str) -> None:
    """Refuse what cannot be parsed this way (pure host code: importable and callable without a GPU).  The priors are needed: they
    enter log w."""
    iw_eval.check_config(cfg, particles)
    if select not in CRITERIA:
        raise ValueError("select must be one of %s, got %r" % (sorted(CRITERIA), select))
    if int(batch_size) < 1:
        raise ValueError("particle parsing needs batch_size >= 1, got %r" % (batch_size,))


class ParticleParser:
    KIND = "particle"

    def __init__(self, cfg: EngineConfig, batch_size: int, particles: int, select: str = "joint", device=None, seed: int = 0,
                 mask_threshold: float = 0.02, keep_layers: bool = False, normalize_steps_prior: bool = True):
        check_arguments(cfg, batch_size, particles, select)
        import torch
        from . import _lib
        if device is not None and torch.device(device).type != "cuda":
            raise _lib.AirHipError("ParticleParser needs a HIP device; there is no CPU fallback")
        from . import hip as H
        from .engine import AIREngine
        self.B, self.K, self.select = int(batch_size), int(particles), select
        self.R = self.B                                       # rows of the parse (what ParseScorer binds to)
        self.mask_threshold = float(mask_threshold)
        self.normalize_steps_prior = bool(normalize_steps_prior)
        self.engine = AIREngine(iw_eval.inner_config(cfg), self.B * self.K, device=device, seed=seed, keep_canvas_steps=False)
        eng, dev = self.engine, self.engine.device
        self.T = eng.T
        B, K, T, A = self.B, self.K, self.T, int(cfg.n_appearance)
        (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
        self.n_bands = int(H.lib().air_canvas_unroll_bands(B, int(Hi)))          # of the B-row render, not of the K * B-row engine
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.obs = z((B, Hi * Wi))
            self.log_weights, self.log_q, self.num_steps = z((B, K)), z((B, K)), z((B, K), torch.int32)
            self.iw_bound, self.elbo, self.ess, self.num_steps_posterior_iw = z((B,)), z((B,)), z((B,)), z((B, T + 1))
            self.best_particle, self.best_score, self.degenerate = z((B,), torch.int32), z((B,)), z((B,), torch.int32)
            self.num_objects_in = z((B,), torch.int32)
            self.where_sel, self.what_sel, self.presence_prob_sel = z((T, B, 4)), z((T, B, A)), z((T, B))
            self.glimpse_sel = z((T, B, hc, wc))
            self.where_mean, self.where_std, self.presence_iw = z((T, B, 4)), z((T, B, 4)), z((T, B))
        self._ro = ReadOut(H, eng, T, B, A, cfg.img_size, self.n_bands, self.mask_threshold, keep_layers)
        self._ro.alias(self)
        self.layers = self._ro.layers
        eng._sync_param_shadow()                              # (see parse.SceneParser: the bf16 shadow of a parser that never loads)
        self._graphs = {}
        self._H = H
        self._build_tail()
        eng.synchronize()

    # ---- the launches behind the engine's forward plan -----------------------------------------------------------------------
    def _build_tail(self):
        H, eng, cfg = self._H, self.engine, self.engine.cfg
        L, p = H.lib(), H._p
        B, K, T, A = self.B, self.K, self.T, int(cfg.n_appearance)
        R = B * K
        (hc, wc) = cfg.crop_size
        shift_loc = cfg.where_shift_prior[0]
        tail = [
            (L.air_iw_logweight,
             (p(eng.what), p(eng.what_loc), p(eng.what_scale), p(eng.where), p(eng.where_loc), p(eng.where_scale),
              p(eng.presence), p(eng.rec), p(eng.logp), p(eng.prior_dev), T, R, K, A, float(cfg.what_prior[0]),
              float(cfg.what_prior[1]), float(cfg.where_scale_prior[0]), float(cfg.where_scale_prior[1]),
              float("nan") if shift_loc is None else float(shift_loc), float(cfg.where_shift_prior[1]),
              1 if self.normalize_steps_prior else 0, p(self.log_weights), p(self.num_steps)), "air_iw_logweight"),
            (L.air_iw_logposterior,
             (p(eng.what), p(eng.what_loc), p(eng.what_scale), p(eng.where), p(eng.where_loc), p(eng.where_scale),
              p(eng.presence), p(eng.logp), T, R, K, A, p(self.log_q)), "air_iw_logposterior"),
            (L.air_iw_reduce, (p(self.log_weights), p(self.num_steps), T, R, K, p(self.iw_bound), p(self.elbo), p(self.ess),
                               p(self.num_steps_posterior_iw), None, None), "air_iw_reduce"),
            (L.air_particle_select,
             (p(self.log_weights), p(self.log_q), p(self.num_steps), p(eng.where), p(eng.what), p(eng.presence_prob),
              p(eng.gd.out[-1]), T, R, K, A, hc * wc, CRITERIA[self.select], p(self.best_particle), p(self.best_score),
              p(self.num_objects_in), p(self.degenerate), p(self.where_sel), p(self.what_sel), p(self.presence_prob_sel),
              p(self.glimpse_sel)), "air_particle_select"),
            (L.air_particle_spread, (p(self.log_weights), p(self.num_steps), p(eng.where), T, R, K, p(self.where_mean),
                                     p(self.where_std), p(self.presence_iw)), "air_particle_spread"),
            self._ro.objects(self.presence_prob_sel, self.num_objects_in, self.where_sel, self.what_sel),
            *self._ro.tail(self.glimpse_sel, self.where_sel, self.obs)]
        # fresh particles per call: the Philox offset moves behind the forward (a train step moves it in its closing update)
        advance = (L.air_rng_advance, (p(eng.rng_state), ctypes.c_uint64(eng._rng_inc)), "air_rng_advance")
        self._plans = {True: list(eng._plan_fwd_noise) + [advance] + tail, False: list(eng._plan_fwd) + tail}

    def rows(self):
        """the provider protocol (stage.py): the selected particle's rows; where_loc is particle 0's, to be gathered per call"""
        return {"what": self.what_sel, "where": self.where_sel, "glimpse": self.glimpse_sel, "presence_prob": self.presence_prob_sel,
                "obs": self.obs, "where_loc": None, "gather_loc": True, "compacted": False}

    def launch_count(self, sample_noise: bool = True) -> Dict[str, int]:
        """entries of one `parse()` call (air_particle_select is two kernels: arg-max, then the gather; air_parse_objects three)"""
        eng = self.engine
        return {"forward": len(eng._plan_fwd_noise if sample_noise else eng._plan_fwd), "rng_advance": 1 if sample_noise else 0,
                "iw": 3, "particle": 2, "parse_objects": 1, "parse_render": 1, "rec_sum": 1}

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def load_from(self, train_engine):
        """device-to-device copy of another engine's parameters (+ the bf16 shadow), its step counter and run-time switches"""
        iw_eval.load_inner_engine(self, train_engine)

    def load_parameters(self, named):
        self.engine.load_parameters(named)

    def set_global_step(self, step: int):
        self.engine.set_global_step(step)

    def update_config(self, **changes) -> bool:
        """run-time switches of the inner engine (AIREngine.KNOBS); the parse graphs are re-captured when one changed"""
        had = bool(self._graphs)
        if had:
            self.engine.synchronize()
        if not self.engine.update_config(**changes):
            return False
        self.release_graphs()
        self._build_tail()
        if had:
            self.capture()
        return True

    # ---- graphs -------------------------------------------------------------------------------------------------------------
    def capture(self):
        """noise + forward + every read-out as ONE hipGraph per variant (fresh / kept noise); `parse` replays the one it needs"""
        self.release_graphs()
        self.engine.synchronize()
        for key, plan in self._plans.items():
            self._graphs[key] = self.engine._capture_plans([plan])

    def release_graphs(self):
        destroy_graphs(self._graphs.values())
        self._graphs = {}

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def parse(self, obs, sample_noise: bool = True):
        """obs [B, H, W] (or [B, H*W]); sample_noise=False keeps the engine's noise buffers as they are (tests).  Returns device
        tensors that the NEXT call overwrites: every key of SceneParser.parse at B rows -- what, where, glimpse and presence_prob are
        the selected particle's rows, num_objects = its count, count_prob = q(that count), num_steps_posterior = q(n | x) -- and
          best_particle [B] int32, best_score [B], degenerate [B] int32 (1: every score was NaN), log_weights, log_q [B, K],
          num_steps [B, K] int32, iw_bound, ess [B], num_steps_posterior_iw [B, T+1], where_mean, where_std [T, B, 4],
          presence_iw [T, B].
        The work runs on the engine's stream; on return the caller's current stream is ordered after it (a device-side wait, no host
        synchronisation), so torch code on that stream may read the results right away, and the next call waits for such readers
        before it overwrites them."""
        import torch
        eng, B, K, T = self.engine, self.B, self.K, self.T
        obs = torch.as_tensor(obs)
        if obs.shape[0] != B or obs.numel() != B * eng.obs.shape[1]:
            raise ValueError("expected %d images of %d pixels, got %s" % (B, eng.obs.shape[1], tuple(obs.shape)))
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):                   # the B-row copy, then its K-fold tiling (a broadcast copy)
            self.obs.copy_(obs.reshape(B, -1), non_blocking=True)
            eng.obs.view(B, K, -1).copy_(self.obs.reshape(B, 1, -1).expand(B, K, -1), non_blocking=True)
        if obs.is_cuda:
            obs.record_stream(eng.stream)
        key = bool(sample_noise)
        eng._replay_or_run(self._graphs.get(key), self._plans[key])
        eng.wait_for_engine()
        out = self._ro.result(self.glimpse_sel)
        out.update({"num_steps_posterior": eng.q_n.view(B, K, T + 1)[:, 0], "presence_prob": self.presence_prob_sel,
                    "what": self.what_sel, "where": self.where_sel,
                    "best_particle": self.best_particle, "best_score": self.best_score, "degenerate": self.degenerate,
                    "log_weights": self.log_weights, "log_q": self.log_q, "num_steps": self.num_steps, "iw_bound": self.iw_bound,
                    "ess": self.ess, "num_steps_posterior_iw": self.num_steps_posterior_iw, "where_mean": self.where_mean,
                    "where_std": self.where_std, "presence_iw": self.presence_iw})
        if self.layers is not None:
            out["layers"] = self.layers
        return out

    def synchronize(self):
        self.engine.synchronize()
