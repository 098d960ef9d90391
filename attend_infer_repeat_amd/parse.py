"""Scene parsing of a trained AIR on the device: image -> list of objects, boxes and instance masks, deterministically.

    n^ = argmax_n q(n | x),   what_t = E_q[what_t],   where_t = E_q[where_t]   (t = 0 .. T-1)

Inference at the mode.  The LSTM never sees the samples, so the presence probabilities -- and with them q(n | x) -- depend on the
image alone, and every step's latents and glimpse are computed whether or not the step is present.  One pass of the engine's own
forward plan with eps_where = eps_what = 0 and u_pres = -1 everywhere (u < p then holds for every p >= 0: the engine's presence
is all ones, nothing is masked upstream) therefore yields what = what_loc, where = where_loc (after the guard_eps rule of the
sampled transform) for all T steps and the exact q(n).  The parse is a read-out behind it.

`SceneParser` owns an ordinary AIREngine at `batch_size` rows, runs that engine's forward plan unchanged (without its noise
entry) and appends the launches of libair_hip.so that include/air_hip.h describes:

  air_parse_objects  count (the smallest n attaining max_n m_n in float64, or the caller's counts clipped to 0..T), presence
                     [t < n^], score [q(n > t)], boxes (evaluation.attention_box in fp32), the flat object table
                     (offsets = exclusive scan of the counts; image-major, step order inside an image; capacity T * R rows, rows from
                     offsets[R] on are not written);
  air_parse_render   canvas = sum_{t < n^} st_write(glimpse_t, where_t), reconstruction = mult * canvas, the reconstruction term
                     against obs in row bands, owner (int8: which object a pixel belongs to, -1 = background; the smallest step
                     attaining max_t mult * layer_t if that is > mask_threshold), area (pixels owned), optionally the layers;
  air_sum_leading    the band shares of the reconstruction term, added in band order.

Forward and read-outs are one hipGraph per variant (model counts / given counts) after `capture()`.  Known waste, deliberate for
now: the forward plan still writes an all-present canvas and its reconstruction sum; the parse discards both.
"""
from typing import Dict

from .engine_config import EngineConfig
from .iw_eval import inner_config, load_inner_engine
from .launch import destroy_graphs
from .stage import ReadOut, engine_rows


def check_config(cfg: EngineConfig) -> None:
    """Refuse what has no count to take the mode of (pure host code: importable and callable without a GPU).  Priors left at
    None are fine: no prior enters."""
    if not cfg.discrete_steps:
        raise ValueError("scene parsing needs discrete_steps=True: with continuous steps there is no count posterior to take "
                         "the mode of")


class SceneParser:
    KIND = "scene"

    def __init__(self, cfg: EngineConfig, batch_size: int, device=None, seed: int = 0, mask_threshold: float = 0.02,
                 keep_layers: bool = False):
        check_config(cfg)
        if int(batch_size) < 1:
            raise ValueError("scene parsing needs batch_size >= 1, got %r" % (batch_size,))
        import torch
        from . import _lib
        if device is not None and torch.device(device).type != "cuda":
            raise _lib.AirHipError("SceneParser needs a HIP device; there is no CPU fallback")
        from . import hip as H
        from .engine import AIREngine
        self.R = int(batch_size)
        self.mask_threshold = float(mask_threshold)
        self.engine = AIREngine(inner_config(cfg), self.R, device=device, seed=seed, keep_canvas_steps=False)
        eng, dev = self.engine, self.engine.device
        self.T = eng.T
        with torch.cuda.device(dev):
            self.num_objects_in = torch.zeros((self.R,), dtype=torch.int32, device=dev)
        self._ro = ReadOut(H, eng, self.T, self.R, cfg.n_appearance, cfg.img_size, eng.n_bands, self.mask_threshold, keep_layers)
        self._ro.alias(self)
        self.layers = self._ro.layers
        # bf16 data path: the engine's constructor zero-fills the parameter shadow on the caller's stream and converts into it on its own
        # stream without ordering the two; it has synchronised the device since, so converting once more here leaves the right shadow
        # (a parser that never loads parameters -- tools/parse_bench.py -- otherwise sometimes kept a zeroed one)
        eng._sync_param_shadow()
        # the mode: zero latent noise, every presence draw succeeds (set once; the plans below never run the noise entry)
        eng.set_noise(torch.zeros_like(eng.eps_where), torch.zeros_like(eng.eps_what), torch.full_like(eng.u_pres, -1.0))
        self._graphs = {}
        self._H = H
        self._build_tail()
        eng.synchronize()

    # ---- the launches behind the engine's forward plan -----------------------------------------------------------------------
    def _build_tail(self):
        eng, ro = self.engine, self._ro
        tail = lambda given: [ro.objects(eng.presence_prob, self.num_objects_in if given else None, eng.where, eng.what)] + \
            ro.tail(eng.gd.out[-1], eng.where, eng.obs)
        self._plans = {given: list(eng._plan_fwd) + tail(given) for given in (False, True)}

    def rows(self):
        """the provider protocol (stage.py): the parse is left in the engine's own buffers"""
        return engine_rows(self.engine)

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call (air_parse_objects is three kernels: count, scan, table; air_parse_render zeroes `area` in
        front of its kernel)"""
        return {"forward": len(self.engine._plan_fwd), "parse_objects": 1, "parse_render": 1, "rec_sum": 1}

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def load_from(self, train_engine):
        """device-to-device copy of another engine's parameters (+ the bf16 shadow), its step counter and run-time switches"""
        load_inner_engine(self, train_engine)

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
        """forward + air_parse_objects + air_parse_render + the band sum as ONE hipGraph per variant (model counts / given counts)"""
        self.release_graphs()
        self.engine.synchronize()
        for key, plan in self._plans.items():
            self._graphs[key] = self.engine._capture_plans([plan])

    def release_graphs(self):
        destroy_graphs(self._graphs.values())
        self._graphs = {}

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def parse(self, obs, num_objects=None):
        """obs [R, H, W] (or [R, H*W]).  num_objects: an int or [R] counts to use instead of the mode of q(n | x) (clipped to 0..T).
        Returns device tensors that the NEXT call overwrites:
          num_objects [R] int32, count_prob [R] (q(n^)), num_steps_posterior [R, T+1] (q(n | x)), presence_prob [T, R],
          presence, score [T, R], boxes [T, R, 4] (left, top, width, height), what [T, R, A], where [T, R, 4], glimpse [T, R, h, w]
          (the decoder's raw output), offsets [R+1] int32, obj_image, obj_step [T*R] int32, obj_box [T*R, 4], obj_score [T*R],
          obj_where [T*R, 4], obj_what [T*R, A] (rows below offsets[R] are objects, the rest is stale), reconstruction [R, H, W],
          rec [R], owner [R, H, W] int8 (-1 = background), area [T, R] int32, and layers [T, R, H, W] with keep_layers.
        The work runs on the engine's stream; on return the caller's current stream is ordered after it (a device-side wait, no host
        synchronisation), so torch code on that stream may read the results right away, and the next call waits for such readers
        before it overwrites them."""
        import torch
        eng, R = self.engine, self.R
        obs = torch.as_tensor(obs)
        if obs.shape[0] != R or obs.numel() != R * eng.obs.shape[1]:
            raise ValueError("expected %d images of %d pixels, got %s" % (R, eng.obs.shape[1], tuple(obs.shape)))
        n = None
        if num_objects is not None:
            n = torch.as_tensor(num_objects)
            if n.numel() not in (1, R):
                raise ValueError("num_objects: one count, or one per image (%d), got shape %s" % (R, tuple(n.shape)))
        eng.wait_for_caller()
        with torch.cuda.stream(eng.stream):
            eng.obs.copy_(obs.reshape(R, -1), non_blocking=True)
            if n is not None:
                self.num_objects_in.copy_(n.reshape(-1).expand(R), non_blocking=True)
        for t in (obs, n):
            if t is not None and t.is_cuda:
                t.record_stream(eng.stream)
        key = n is not None
        eng._replay_or_run(self._graphs.get(key), self._plans[key])
        eng.wait_for_engine()
        out = self._ro.result(eng.gd.out[-1])
        out.update({"num_steps_posterior": eng.q_n, "presence_prob": eng.presence_prob, "what": eng.what, "where": eng.where})
        if self.layers is not None:
            out["layers"] = self.layers
        return out

    def synchronize(self):
        self.engine.synchronize()
