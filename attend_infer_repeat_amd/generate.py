"""Scenes from the generative model of a trained AIR on the device.

    n ~ pi(n),   z_t = [t < n],   what_t ~ N(what_prior),   where_t = [sx, tx, sy, ty] ~ N(scale prior) x N(shift prior),
    canvas = sum_t z_t * st_write(decoder(what_t), where_t),   x ~ N(output_multiplier * canvas, output_std)

`SceneSampler` owns the decoder weights, its latent / glimpse / canvas buffers, a Philox state, a float64 count table and a
stream -- it is not an AIREngine.  One `sample()` is a fixed list of launches of libair_hip.so (include/air_hip.h):
air_rng_fill (latent noise), air_prior_latents (the ancestral draw), the decoder layers (air_linear_fwd, or air_gemm_bf16 with
the matching epilogues under mfma_dtype="bf16": the rounding of the engine's decoder), air_canvas_unroll_fwd without an
observation, air_observe (mean and the noisy observation; the pixel noise is drawn in registers and never stored) and
air_rng_advance.  After `capture()` the chain replays as one hipGraph.  `decode()` runs the same chain from the decoder on for
latents the caller supplies (traversals, edits of `where`), `dream()` fills a dataset AIREngine.attach_dataset can train on.

Philox bookkeeping of one call at state {seed, offset}: the latent noise takes quads [offset, offset + q_lat), the pixel noise
quads [offset + q_lat, offset + q_lat + q_pix) (air_observe's counter_base = q_lat), the state then moves by q_lat + q_pix.

air_observe and values that are not numbers: a NaN clamp bound switches the clamp off on that side only; a NaN canvas pixel stays NaN
in the mean and leaves a finite clamp as its lower bound (as the upper one when only that is given), with and without noise.
"""
import ctypes
from typing import Dict

from .engine_config import EngineConfig, _mlp_shapes
from .launch import LaunchMixin, destroy_graphs


def check_config(cfg: EngineConfig) -> None:
    """Refuse what defines no generative density (pure host code: importable and callable without a GPU)."""
    if cfg.what_prior is None:
        raise ValueError("scene sampling needs what_prior: without it the model has no generative density over the "
                         "appearance latents")
    if cfg.where_scale_prior is None or cfg.where_shift_prior is None:
        raise ValueError("scene sampling needs where_scale_prior and where_shift_prior: without them the model has no "
                         "generative density over the transform latents")
    if cfg.where_shift_prior[0] is None:
        raise ValueError("scene sampling needs where_shift_prior[0] (the location of the shift prior): a shift prior centred on "
                         "the posterior's own mean defines no stand-alone generative density")


def count_table(count_probs, T: int):
    """the T + 1 non-negative weights of a caller-given count distribution as a list of floats ("uniform": all ones)"""
    if isinstance(count_probs, str):
        if count_probs != "uniform":
            raise ValueError("count_probs: a list / tensor of %d weights, 'uniform' or None, got %r" % (T + 1, count_probs))
        return [1.0] * (T + 1)
    vals = [float(v) for v in (count_probs.reshape(-1).tolist() if hasattr(count_probs, "reshape") else list(count_probs))]
    if len(vals) != T + 1:
        raise ValueError("count_probs: %d weights expected (counts 0..%d), got %d" % (T + 1, T, len(vals)))
    if any(not (v >= 0.0) or v == float("inf") for v in vals) or not sum(vals) > 0.0:
        raise ValueError("count_probs: finite non-negative weights with a positive sum expected, got %r" % (vals,))
    return vals


class SceneSampler(LaunchMixin):
    """count_probs=None: the model's own count prior at the sampler's global step (air_steps_prior: the float64 arithmetic of
    the engine's table, unnormalised geometric weights).  NOTE: under the training script's schedule that table collapses onto
    n = 0 once annealed (nsp_final = 1e-7: p(n = 0) = 1 - 1e-7) -- prior samples of a fully trained model are then empty
    scenes; pass `count_probs` (T + 1 weights, or "uniform") or `sample(num_objects=...)` to look at scenes with objects.
    pixel_noise=False: obs = mean.  clamp=(lo, hi): the observation is clamped (e.g. (0, 1) for image-valued dreams)."""

    def __init__(self, cfg: EngineConfig, n_scenes: int, device=None, seed: int = 0, count_probs=None, pixel_noise: bool = True,
                 clamp=None):
        check_config(cfg)
        if cfg.mfma_dtype not in ("f32", "bf16"):
            raise ValueError("mfma_dtype must be 'f32' or 'bf16', got %r" % (cfg.mfma_dtype,))
        if int(n_scenes) < 1:
            raise ValueError("scene sampling needs n_scenes >= 1, got %r" % (n_scenes,))
        import torch
        from . import _lib
        from . import hip as H
        H.lib()
        self._H = H
        self.cfg = cfg
        self.R, self.T = int(n_scenes), int(cfg.max_steps)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise _lib.AirHipError("SceneSampler needs a HIP device; there is no CPU fallback")
        self.pixel_noise = bool(pixel_noise)
        self.clamp = (float("nan"), float("nan")) if clamp is None else (float(clamp[0]), float(clamp[1]))
        self.output_multiplier = float(cfg.output_multiplier)
        self.global_step = 0
        R, T, A, P, hw = self.R, self.T, int(cfg.n_appearance), cfg.n_pix, cfg.n_crop
        dev = self.device
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.stream = torch.cuda.Stream(device=dev)
            self.shapes = _mlp_shapes(A, cfg.glimpse_decoder_hidden, hw)
            self.params = {}
            gen = torch.Generator(device="cpu").manual_seed(int(seed))
            for i, (k, n) in enumerate(self.shapes):               # Sonnet defaults, as AIREngine.init_parameters
                w = torch.empty((k, n), dtype=torch.float32)
                torch.nn.init.trunc_normal_(w, mean=0.0, std=1.0, a=-2.0, b=2.0, generator=gen)
                self.params["glimpse_decoder/%d/w" % i] = (w * k ** -0.5).to(dev)
                self.params["glimpse_decoder/%d/b" % i] = z((n,))
            # noise: one flat normal buffer [eps_where | eps_what] (both 16-byte aligned), one uniform per scene
            self.noise_normal = z((T * R * 4 + T * R * A,))
            self.eps_where = self.noise_normal[:T * R * 4].view(T, R, 4)
            self.eps_what = self.noise_normal[T * R * 4:].view(T, R, A)
            self.u_n = z((R,))
            self.num_objects_in = z((R,), torch.int32)
            self.what, self.where, self.presence = z((T, R, A)), z((T, R, 4)), z((T, R))
            self.num_objects = z((R,), torch.int32)
            self.act = [z((T * R, n)) for _, n in self.shapes]
            self.glimpse = self.act[-1].view(T, R, *cfg.crop_size)
            self.canvas = z((R, P))
            self.mean, self.obs = z((R,) + tuple(cfg.img_size)), z((R,) + tuple(cfg.img_size))
            self.table = z((T + 1,), torch.float64)
            self.step_dev = z((1,), torch.int64)
            self.rng_state = torch.tensor([int(seed), 0], dtype=torch.int64, device=dev)
        self.q_lat = (self.noise_normal.numel() + 3) // 4 + (R + 3) // 4
        self.q_pix = (R * P + 3) // 4 if self.pixel_noise else 0
        self._graphs = {}
        self._build_plans()
        self.set_count_probs(count_probs)
        self.synchronize()

    # ---- the launch list -----------------------------------------------------------------------------------------------------
    def _build_plans(self):
        H, cfg = self._H, self.cfg
        L, p = H.lib(), H._p
        R, T, A = self.R, self.T, int(cfg.n_appearance)
        (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
        rng = (L.air_rng_fill, (p(self.noise_normal), ctypes.c_size_t(self.noise_normal.numel()), p(self.u_n),
                                ctypes.c_size_t(R), p(self.rng_state)), "air_rng_fill")

        def latents(given_counts):
            return (L.air_prior_latents,
                    (p(self.table), p(self.u_n), p(self.num_objects_in) if given_counts else None, p(self.eps_what),
                     p(self.eps_where), float(cfg.what_prior[0]), float(cfg.what_prior[1]), float(cfg.where_scale_prior[0]),
                     float(cfg.where_scale_prior[1]), float(cfg.where_shift_prior[0]), float(cfg.where_shift_prior[1]),
                     float(cfg.guard_eps), T, R, A, p(self.what), p(self.where), p(self.presence), p(self.num_objects)),
                    "air_prior_latents")
        decoder = []
        x = self.what
        for i, (k, n) in enumerate(self.shapes):                   # ELU on the hidden layers, none on the last (modules.py:86-91)
            last = i == len(self.shapes) - 1
            w, b = self.params["glimpse_decoder/%d/w" % i], self.params["glimpse_decoder/%d/b" % i]
            if cfg.mfma_dtype == "bf16":
                decoder.append((L.air_gemm_bf16, (0, 0, T * R, n, k, p(x), k, p(w), n, p(self.act[i]), n, p(b),
                                                  H.EPI_BIAS if last else H.EPI_BIAS_ELU, None, 0, 0.0, None, None,
                                                  ctypes.c_size_t(0)), "air_gemm_bf16"))
            else:
                decoder.append((L.air_linear_fwd, (p(x), p(w), p(b), p(self.act[i]), T * R, k, n,
                                                   H.ACT_NONE if last else H.ACT_ELU, None, ctypes.c_size_t(0)), "air_linear_fwd"))
            x = self.act[i]
        canvas = (L.air_canvas_unroll_fwd, (p(self.act[-1]), p(self.where), p(self.presence), None, None, p(self.canvas), None,
                                            T, R, Hi, Wi, hc, wc, self.output_multiplier, float(cfg.output_std)),
                  "air_canvas_unroll_fwd")
        n_pix = ctypes.c_size_t(self.canvas.numel())

        def observe(std, obs):                                     # std = 0: no draw; obs = None: the mean alone
            return (L.air_observe, (p(self.canvas), self.output_multiplier, std, p(self.rng_state), ctypes.c_uint64(self.q_lat),
                                    self.clamp[0], self.clamp[1], p(self.mean), p(obs), n_pix), "air_observe")
        advance = (L.air_rng_advance, (p(self.rng_state), ctypes.c_uint64(self.q_lat + self.q_pix)), "air_rng_advance")
        tail = decoder + [canvas, observe(float(cfg.output_std) if self.pixel_noise else 0.0, self.obs), advance]
        self._plans = {"decode": decoder + [canvas, observe(0.0, None)]}
        for noise in (False, True):
            for given in (False, True):
                self._plans[(noise, given)] = ([rng] if noise else []) + [latents(given)] + tail

    def launch_count(self, sample_noise: bool = True) -> Dict[str, int]:
        """entries of one `sample()` call"""
        return {"rng_fill": 1 if sample_noise else 0, "prior_latents": 1, "decoder": len(self.shapes), "canvas": 1, "observe": 1,
                "rng_advance": 1}

    def _launch(self, key):
        self._replay_or_run(self._graphs.get(key), self._plans[key])

    # ---- stream discipline: launch.LaunchMixin (the engine's: work runs on the sampler's stream, whatever enters or leaves is ordered
    #      explicitly)
    wait_for_sampler = LaunchMixin.wait_for_stream

    # ---- parameters and switches -----------------------------------------------------------------------------------------------
    def load_from(self, engine):
        """device-to-device copy of an AIREngine's glimpse_decoder/*, its step counter and its output_multiplier"""
        for k, v in self.params.items():
            if k not in engine.params or tuple(engine.params[k].shape) != tuple(v.shape):
                raise ValueError("the engine's decoder differs in architecture (%s)" % k)
        engine.wait_for_engine()                             # the caller's stream now follows the engine's pending updates
        for k, v in self.params.items():
            self._copy_in(v, engine.params[k])
        self._copy_in(self.step_dev, engine.step_dev)
        self.global_step = int(engine.global_step)
        engine.stream.wait_stream(self.stream)               # ... and its next update follows the copy
        self._set_output_multiplier(float(engine.cfg.output_multiplier))
        self._refresh_table()

    def load_parameters(self, named):
        """glimpse_decoder/<i>/w, /b by name; other names (a full model's parameter dict) are ignored"""
        import torch
        for k, v in named.items():
            if k in self.params:
                self._copy_in(self.params[k], torch.as_tensor(v).to(torch.float32))

    def _set_output_multiplier(self, mult: float):
        if mult == self.output_multiplier:
            return
        had = bool(self._graphs)
        self.synchronize()
        self.release_graphs()
        self.output_multiplier = mult
        self._build_plans()
        if had:
            self.capture()

    def set_global_step(self, step: int):
        """host mirror + the device counter the model's own count table is evaluated at"""
        self.global_step = int(step)
        self._fill_in(self.step_dev, int(step))
        self._refresh_table()

    def set_count_probs(self, count_probs=None):
        """None: the model's own table at the current global step; 'uniform'; or T + 1 non-negative weights (unnormalised is fine)"""
        import torch
        if count_probs is None:
            self.count_probs, self.count_label = None, "model prior at step %d" % self.global_step
            self._refresh_table()
            return
        vals = count_table(count_probs, self.T)
        self.count_probs = vals
        self.count_label = "uniform" if isinstance(count_probs, str) else "[%s]" % ", ".join("%.3g" % v for v in vals)
        self._copy_in(self.table, torch.tensor(vals, dtype=torch.float64))

    def _refresh_table(self):
        if self.count_probs is not None:
            return
        from . import _lib
        cfg, L, p = self.cfg, self._H.lib(), self._H._p
        anneal = {None: 0, "exp": 1, "linear": 2}[cfg.nsp_anneal]
        self.count_label = "model prior at step %d" % self.global_step
        _lib.check(L.air_steps_prior(p(self.step_dev), anneal, float(cfg.nsp_init), float(cfg.nsp_final), float(cfg.nsp_steps),
                                     float(cfg.nsp_hold_init), float(cfg.nsp_steps_div), p(self.table), self.T, self._sp()),
                   "air_steps_prior")

    def set_noise(self, eps_what, eps_where, u_n):
        """latent noise for `sample(sample_noise=False)`: eps_what [T, R, A], eps_where [T, R, 4], u_n [R]"""
        self._copy_in(self.eps_what, eps_what)
        self._copy_in(self.eps_where, eps_where)
        self._copy_in(self.u_n, u_n)

    # ---- graphs ----------------------------------------------------------------------------------------------------------------
    def capture(self):
        """every variant of the chain (fresh / kept latent noise, drawn / given counts, decode) as ONE hipGraph each"""
        self.release_graphs()
        self.synchronize()
        for key, plan in self._plans.items():
            self._graphs[key] = self._capture_plans([plan])

    def release_graphs(self):
        destroy_graphs(self._graphs.values())
        self._graphs = {}

    # ---- the three entries -----------------------------------------------------------------------------------------------------
    def sample(self, num_objects=None, sample_noise: bool = True):
        """n_scenes scenes.  num_objects: an int or [R] counts to condition on (clipped to 0..T) instead of drawing them.
        sample_noise=False keeps the latent noise `set_noise` left (the pixel noise is always fresh).  Returns device tensors
        that the NEXT call overwrites: obs, mean [R, H, W], what [T, R, A], where [T, R, 4], presence [T, R], num_objects [R]
        (int32), glimpse [T, R, h, w] (the decoder's output, as the canvas receives it).  The work runs on the sampler's stream;
        on return the caller's current stream is ordered after it (a device-side wait, no host synchronisation), and the next
        call waits for such readers before it overwrites the results."""
        import torch
        self.wait_for_caller()
        if num_objects is not None:
            n = torch.as_tensor(num_objects)
            if n.numel() not in (1, self.R):
                raise ValueError("num_objects: one count, or one per scene (%d), got shape %s" % (self.R, tuple(n.shape)))
            with torch.cuda.stream(self.stream):
                self.num_objects_in.copy_(n.reshape(-1).expand(self.R), non_blocking=True)
            if n.is_cuda:
                n.record_stream(self.stream)
        self._launch((bool(sample_noise), num_objects is not None))
        self.wait_for_sampler()
        return {"obs": self.obs, "mean": self.mean, "what": self.what, "where": self.where, "presence": self.presence,
                "num_objects": self.num_objects, "glimpse": self.glimpse}

    def decode(self, what, where, presence):
        """mean [R, H, W] and glimpse [T, R, h, w] of caller-given latents (what [T, R, A], where [T, R, 4], presence [T, R] or
        [T, R, 1]); no pixel noise, the Philox state does not move.  Same stream contract as `sample`."""
        import torch
        for name, t, dst in (("what", what, self.what), ("where", where, self.where), ("presence", presence, self.presence)):
            if torch.as_tensor(t).numel() != dst.numel():
                raise ValueError("%s: %s expected, got %s" % (name, tuple(dst.shape), tuple(torch.as_tensor(t).shape)))
            self._copy_in(dst, t)
        self._launch("decode")
        self.wait_for_sampler()
        return {"mean": self.mean, "glimpse": self.glimpse}

    def dream(self, n_items: int):
        """(data [N, H, W] float32, nums [N] int32) of N generated scenes, drawn n_scenes at a time: what
        AIREngine.attach_dataset(data) takes.  Allocated on the caller's stream; complete when that stream reaches this point."""
        import torch
        N, R = int(n_items), self.R
        with torch.cuda.device(self.device):
            data = torch.empty((N,) + tuple(self.cfg.img_size), dtype=torch.float32, device=self.device)
            nums = torch.empty((N,), dtype=torch.int32, device=self.device)
        for lo in range(0, N, R):
            k = min(R, N - lo)
            out = self.sample()
            data[lo:lo + k].copy_(out["obs"][:k])
            nums[lo:lo + k].copy_(out["num_objects"][:k])
        self.wait_for_caller()                               # the sampler's next launch follows the last copies
        return data, nums
