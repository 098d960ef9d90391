"""K-particle importance-weighted evaluation of a trained AIR model on the device.

    L_K(x) = log (1/K) sum_k w_k,   w_k = p(x, z_k) / q(z_k | x),   z_k ~ q(. | x)

together with the plain ELBO of the same particles, the effective sample size and the self-normalised posterior over the
object count.  `ImportanceEvaluator` owns an ordinary AIREngine at K * B rows (row r = b * K + k: the particles of an image
are adjacent), runs that engine's own forward plan unchanged and appends two launches of libair_hip.so (include/air_hip.h):
air_iw_logweight turns the forward's buffers into log w per row, air_iw_reduce folds the K log-weights of every image and
keeps float64 running totals on the device.  Noise, forward and both read-outs are one hipGraph after `capture()`.

With z_t the sampled cumulative presence and n = sum_t z_t:

    log w = -rec_loss_per_sample + log pi(n) - log q(n)
            + sum_t z_t [ sum_a (log p(what_ta) - log q(what_ta)) + sum_j (log p(where_tj) - log q(where_tj)) ]

The mask z_t is exact: the LSTM never sees the samples, so the presence probabilities do not depend on what / where, and
latents of absent steps reach neither the canvas nor a later step -- they integrate out of numerator and denominator.
This is a property of the model: use_prior, nsp_weight, nsp_analytic, use_reinforce, l2_weight and decay_rate do not enter.

air_iw_reduce on log-weights that are not finite (held by tests/test_readout_kernels.py; the shift of the logsumexp is 0 when the
maximum is infinite, and a NaN never becomes the maximum):

    all K weights -inf   iw_bound = -inf   elbo = -inf   ess = NaN   q_n = NaN for every count
    one weight +inf      iw_bound = +inf   elbo = +inf   ess = NaN   q_n = NaN at that particle's count, 0 at the others
    one weight NaN       iw_bound = NaN    elbo = NaN    ess = NaN   q_n = NaN for every count

Single particles at -inf have a weight of exactly 0 and only move elbo (to -inf).  A num_steps outside 0..T is counted in no q_n, which
then sums to less than 1 by that particle's share.  The running totals add such values as they are.
"""
import ctypes
import dataclasses
from typing import Dict

from .engine_config import EngineConfig
from .launch import destroy_graphs


def check_config(cfg: EngineConfig, particles: int) -> None:
    """Refuse what has no importance weight (pure host code: importable and callable without a GPU)."""
    if int(particles) < 1:
        raise ValueError("importance-weighted evaluation needs particles >= 1, got %r" % (particles,))
    if not cfg.discrete_steps:
        raise ValueError("importance-weighted evaluation needs discrete_steps=True: with continuous steps there is no "
                         "discrete chain of presences to weigh")
    if cfg.what_prior is None:
        raise ValueError("importance-weighted evaluation needs what_prior: without it the model has no generative density "
                         "over the appearance latents")
    if cfg.where_scale_prior is None or cfg.where_shift_prior is None:
        raise ValueError("importance-weighted evaluation needs where_scale_prior and where_shift_prior: without them the "
                         "model has no generative density over the transform latents")


def inner_config(cfg: EngineConfig) -> EngineConfig:
    """The configuration of the K * B-row engine: the model as it is, without the training-loss extras (its forward plan then
    ends at the reconstruction sum: no baseline MLP, no NVIL)."""
    return dataclasses.replace(cfg, use_reinforce=False, decay_rate=None, l2_weight=0.0)


def load_inner_engine(owner, train_engine):
    """`owner.engine` takes another engine's parameters (+ the bf16 shadow), its step counter and run-time switches, device to
    device; the switches go through `owner.update_config` (which re-captures the owner's graphs when one changed).  Shared by
    ImportanceEvaluator and parse.SceneParser."""
    eng = owner.engine
    if train_engine.n_total != eng.n_total or dict(train_engine.param_offsets) != dict(eng.param_offsets):
        raise ValueError("the engines differ in architecture (flat parameter layout)")
    knobs = {k: getattr(train_engine.cfg, k) for k in eng.KNOBS if k != "use_prior"}
    owner.update_config(**knobs)
    train_engine.wait_for_engine()                           # the caller's stream now follows the training engine's pending updates
    eng._copy_in(eng.flat_params, train_engine.flat_params)
    eng._copy_in(eng.step_dev, train_engine.step_dev)
    eng.global_step = int(train_engine.global_step)
    eng._sync_param_shadow()
    train_engine.stream.wait_stream(eng.stream)              # ... and its next update follows the copy


class ImportanceEvaluator:
    def __init__(self, cfg: EngineConfig, batch_size: int, particles: int, device=None, seed: int = 0,
                 normalize_steps_prior: bool = True):
        check_config(cfg, particles)
        import torch
        from . import hip as H
        from .engine import AIREngine
        self.B, self.K = int(batch_size), int(particles)
        self.R = self.B * self.K
        self.normalize_steps_prior = bool(normalize_steps_prior)
        self.engine = AIREngine(inner_config(cfg), self.R, device=device, seed=seed, keep_canvas_steps=False)
        eng, dev = self.engine, self.engine.device
        self.T = eng.T
        B, K, T = self.B, self.K, self.T
        with torch.cuda.device(dev):
            self.log_weights = torch.zeros((B, K), dtype=torch.float32, device=dev)
            self.num_steps = torch.zeros((B, K), dtype=torch.int32, device=dev)
            self.iw_bound = torch.zeros(B, dtype=torch.float32, device=dev)
            self.elbo = torch.zeros(B, dtype=torch.float32, device=dev)
            self.ess = torch.zeros(B, dtype=torch.float32, device=dev)
            self.num_steps_posterior = torch.zeros((B, T + 1), dtype=torch.float32, device=dev)
            self.gt_steps = torch.zeros(B, dtype=torch.int32, device=dev)
            self.acc = torch.zeros(8, dtype=torch.float64, device=dev)
        self._graphs = {}
        self._calls_without_counts = 0
        self._H = H
        self._build_tail()
        eng.synchronize()

    # ---- the two launches behind the engine's forward plan ------------------------------------------------------------------
    def _build_tail(self):
        H, eng, cfg = self._H, self.engine, self.engine.cfg
        L, p = H.lib(), H._p
        shift_loc = cfg.where_shift_prior[0]
        logweight = (L.air_iw_logweight,
                     (p(eng.what), p(eng.what_loc), p(eng.what_scale), p(eng.where), p(eng.where_loc), p(eng.where_scale),
                      p(eng.presence), p(eng.rec), p(eng.logp), p(eng.prior_dev), self.T, self.R, self.K,
                      int(cfg.n_appearance), float(cfg.what_prior[0]), float(cfg.what_prior[1]),
                      float(cfg.where_scale_prior[0]), float(cfg.where_scale_prior[1]),
                      float("nan") if shift_loc is None else float(shift_loc), float(cfg.where_shift_prior[1]),
                      1 if self.normalize_steps_prior else 0, p(self.log_weights), p(self.num_steps)), "air_iw_logweight")

        def reduce(with_counts):
            return (L.air_iw_reduce, (p(self.log_weights), p(self.num_steps), self.T, self.R, self.K, p(self.iw_bound),
                                      p(self.elbo), p(self.ess), p(self.num_steps_posterior),
                                      p(self.gt_steps) if with_counts else None, p(self.acc)), "air_iw_reduce")
        # fresh particles per call: the Philox offset moves behind the forward (a train step moves it in its closing update)
        advance = (L.air_rng_advance, (p(eng.rng_state), ctypes.c_uint64(eng._rng_inc)), "air_rng_advance")
        self._plans = {}
        for noise in (False, True):
            fwd = eng._plan_fwd_noise if noise else eng._plan_fwd
            for counts in (False, True):
                self._plans[(noise, counts)] = list(fwd) + ([advance] if noise else []) + [logweight, reduce(counts)]

    def launch_count(self, sample_noise: bool = True) -> Dict[str, int]:
        """entries of one evaluation (air_iw_reduce is two kernels: per image, then the totals)"""
        eng = self.engine
        return {"forward": len(eng._plan_fwd_noise if sample_noise else eng._plan_fwd), "rng_advance": 1 if sample_noise else 0,
                "iw": 2}

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def load_from(self, train_engine):
        """device-to-device copy of another engine's parameters (+ the bf16 shadow), its step counter and run-time switches"""
        load_inner_engine(self, train_engine)

    def load_parameters(self, named):
        self.engine.load_parameters(named)

    def set_global_step(self, step: int):
        self.engine.set_global_step(step)

    def update_config(self, **changes) -> bool:
        """run-time switches of the inner engine (AIREngine.KNOBS); the evaluation graphs are re-captured when one changed"""
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
        """noise + forward + air_iw_logweight + air_iw_reduce as ONE hipGraph per variant (fresh / kept noise, with / without
        ground-truth counts); `evaluate` replays the one it needs"""
        self.release_graphs()
        self.engine.synchronize()
        for key, plan in self._plans.items():
            self._graphs[key] = self.engine._capture_plans([plan])

    def release_graphs(self):
        destroy_graphs(self._graphs.values())
        self._graphs = {}

    # ---- evaluation ---------------------------------------------------------------------------------------------------------
    def evaluate(self, obs, nums=None, sample_noise: bool = True):
        """obs [B, H, W] (or [B, H*W]); nums: the true object count per image [B] (any numeric dtype), optional.  Returns device
        tensors that the NEXT call overwrites.  The work runs on the engine's stream; on return the caller's current stream is
        ordered after it (a device-side wait, no host synchronisation), so torch code on that stream may read the results right
        away, and the next call waits for such readers before it overwrites them."""
        import torch
        eng, B, K = self.engine, self.B, self.K
        obs = torch.as_tensor(obs)
        if obs.shape[0] != B or obs.numel() != B * eng.obs.shape[1]:
            raise ValueError("expected %d images of %d pixels, got %s" % (B, eng.obs.shape[1], tuple(obs.shape)))
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):                   # K-fold tiling: a broadcast copy on the engine's stream
            eng.obs.view(B, K, -1).copy_(obs.reshape(B, 1, -1).expand(B, K, -1), non_blocking=True)
            if nums is not None:
                nums = torch.as_tensor(nums)
                if nums.numel() != B:
                    raise ValueError("nums: one object count per image expected, got shape %s" % (tuple(nums.shape),))
                self.gt_steps.copy_(nums.reshape(B), non_blocking=True)
        for t in (obs, nums):
            if t is not None and t.is_cuda:
                t.record_stream(eng.stream)
        key = (bool(sample_noise), nums is not None)
        if nums is None:
            self._calls_without_counts += 1
        eng._replay_or_run(self._graphs.get(key), self._plans[key])
        eng.wait_for_engine()
        return {"log_weights": self.log_weights, "num_steps": self.num_steps, "iw_bound": self.iw_bound, "elbo": self.elbo,
                "ess": self.ess, "num_steps_posterior": self.num_steps_posterior}

    def reset(self):
        self.engine._fill_in(self.acc, 0.0)
        self._calls_without_counts = 0

    def totals(self) -> Dict[str, float]:
        """per-image means over every image evaluated since `reset()` (the device block holds the float64 sums and the image
        count): one sync, one 64-byte copy.  num_step_acc is NaN unless every call came with the true counts."""
        self.engine.synchronize()
        a = self.acc.cpu().tolist()
        n = a[4]
        mean = lambda v: v / n if n > 0 else float("nan")
        acc = mean(a[3]) if self._calls_without_counts == 0 else float("nan")
        return {"iw_bound": mean(a[0]), "elbo": mean(a[1]), "ess": mean(a[2]), "num_step_acc": acc, "n_images": float(n)}

    def synchronize(self):
        self.engine.synchronize()
