"""Refining a scene parse on the device: a fixed number of gradient-ascent iterations on log p(x, z) in the continuous latents.

    z_0 = the bound parser's parse,   z_{i+1} = Adam step on J(z_i),   result = the z_i with the largest J (i = 0 .. steps)

    J_b(z) = -rec_b(x | mult * canvas(decode(what), where, presence))
             + sum_{t<n} [ sum_a log N(what_ta | what_prior) + sum_{j in 0,2} log N(where_tj | where_scale_prior)
                                                             + sum_{j in 1,3} log N(where_tj | where_shift_prior) ]

Semi-amortised inference: the inference network's answer (parse.SceneParser at the mode, or particle_parse.ParticleParser's best of K
samples) is the starting point; the generative model's own joint density is then climbed.  n = the count of the start parse and the
presence chain with it stay fixed; log pi(n) is constant and left out.  A where_shift_prior without `loc` is centred on the start
parse's where_loc, held constant (the NaN convention of air_iw_logweight; for a ParticleParser that is particle 0's where_loc -- the
LSTM never sees the samples, so the particles of an image share it).  The mask t < n is exact for the reason iw_eval gives.

`ParseRefiner` owns no engine: it binds to a parser, runs the parser's own `parse()` and then, on the same engine stream, its own
launch list of libair_hip.so entries (include/air_hip.h), captured as ONE hipGraph by `capture()`:

  air_tile_rows x2, air_fill       the start latents into the refiner's buffers, the Adam moments to zero;
  per iteration i = 0 .. steps
    air_linear_fwd x L             the glimpse decoder on T * B rows (iteration 0 evaluates the start parse as the parser left it -- its
                                   own glimpse rows reach the canvas and the keep rule -- and runs the decoder only for the hidden
                                   activations its backward needs; not at all when steps = 0);
    air_canvas_unroll_fwd_banded   final_canvas and the band shares of the reconstruction term;
    if i < steps: air_canvas_unroll_bwd (loss_scale = 1: gradients of sum_b rec_b), air_gemm x L with tb = 1 (AIR_EPI_MUL_DELU on the
                  hidden layers: the decoder's dX chain), air_refine_step(do_update = 1);
    else:         air_refine_step(do_update = 0);
  air_parse_objects (given counts), air_parse_render, air_sum_leading   on the best rows, into the refiner's own buffers.

One exception to "one hipGraph": behind a ParticleParser with a shift prior given without `loc`, particle 0's where_loc rows are
gathered by a strided device copy on the engine stream BEFORE the launch list (the library has no strided-gather entry, and
air_refine_step takes where_loc as [T, B, 4]); every other configuration reads the parser's where_loc in place.

air_refine_step is the one new kernel: the objective, the keep rule (iteration 0 is always taken, later ones iff J is not NaN and
exceeds the best so far -- strictly, so the result is never worse than the start parse and the earliest iteration wins a tie) and
the Adam update of the rows t < n.  `reference_step` restates it in numpy float64.
"""
import ctypes
import math
from typing import Dict

from . import iw_eval
from .engine_config import EngineConfig
from .stage import BoundStage, ReadOut, prior_arguments

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
DEFAULT_LR = (1e-1, 1e-2)     # (lr_what, lr_where): the largest mean objective gain at N = 16 in the sweep of profiles/refine.txt


def check_arguments(cfg: EngineConfig, steps: int, lr_what: float, lr_where: float, beta1: float = 0.9, beta2: float = 0.999,
                    eps: float = 1e-8) -> None:
    """Refuse what cannot be refined this way (pure host code: importable and callable without a GPU).  The priors are needed: they
    are the latent terms of log p(x, z)."""
    if int(steps) != steps or int(steps) < 0:
        raise ValueError("refinement needs steps >= 0 (an integer), got %r" % (steps,))
    for name, lr in (("lr_what", lr_what), ("lr_where", lr_where)):
        if not (float(lr) >= 0.0) or math.isinf(float(lr)):
            raise ValueError("%s must be a finite learning rate >= 0, got %r" % (name, lr))
    for name, beta in (("beta1", beta1), ("beta2", beta2)):
        if not (0.0 <= float(beta) < 1.0):
            raise ValueError("%s must lie in [0, 1), got %r" % (name, beta))
    if not (float(eps) > 0.0):
        raise ValueError("eps must be > 0, got %r" % (eps,))
    iw_eval.check_config(cfg, 1)
    if cfg.mfma_dtype == "bf16":
        raise ValueError('refinement with mfma_dtype="bf16" is out of scope: the decoder would round its operands to bf16 in every '
                         "iteration of a gradient loop whose steps are smaller than that rounding; use the f32 data path")


def _log_normal(x, loc, scale):
    import numpy as np
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = (x - loc) / scale
        return -0.5 * z * z - np.log(scale) - HALF_LOG_2PI


def reference_step(what, where, glimpse, presence, rec_parts, dwhat, dwhere, where_loc, priors, m_what, v_what, m_where, v_where,
                   lr_what, lr_where, beta1, beta2, eps, c1, c2, guard_eps, iter, do_update, best=None):
    """air_refine_step restated in plain numpy float64 (include/air_hip.h states the rule; the tests and DESIGN section 13 refer to this).
    Arrays as the kernel takes them (what [T, B, A], where [T, B, 4], glimpse [T, B, G], presence [T, B], rec_parts [n_bands, B], ...);
    priors = (what_loc, what_scale, scale_loc, scale_scale, shift_loc or None / NaN, shift_scale).  `best` = the dict a previous call
    returned under "best" (J, iter, what, where, glimpse), or None before iteration 0.  Nothing is modified in place.  Returns
      J [B] float64, take [B] bool, what, where, m_what, v_what, m_where, v_where (float64; the inputs' values where nothing moved),
      best = {"J", "iter", "what", "where", "glimpse"} after the keep rule."""
    import numpy as np
    f = lambda a: None if a is None else np.array(a, dtype=np.float64)
    what, where, glimpse, presence, rec_parts = f(what), f(where), f(glimpse), f(presence), f(rec_parts)
    T, B, A = what.shape
    w_loc, w_scale, s_loc, s_scale, h_loc, h_scale = [float("nan") if v is None else float(v) for v in priors]
    n = np.cumprod(presence > 0.5, axis=0).sum(0).astype(np.int64)                     # leading ones
    mask = (np.arange(T)[:, None] < n[None, :])                                         # [T, B]
    mu_where = np.empty_like(where)
    mu_where[..., 0::2] = s_loc
    mu_where[..., 1::2] = f(where_loc)[..., 1::2] if math.isnan(h_loc) else h_loc
    sd_where = np.empty_like(where)
    sd_where[..., 0::2], sd_where[..., 1::2] = s_scale, h_scale

    rec = np.zeros(B)
    for k in range(rec_parts.shape[0]):
        rec = rec + rec_parts[k]
    lp = _log_normal(what, w_loc, w_scale).sum(-1) + _log_normal(where, mu_where, sd_where).sum(-1)          # [T, B]
    with np.errstate(invalid="ignore"):
        J = -rec + np.where(mask, lp, 0.0).sum(0)

    if best is None or iter == 0:
        take = np.ones(B, bool)
        best = {"J": np.full(B, np.nan), "iter": np.zeros(B, np.int64), "what": np.zeros_like(what), "where": np.zeros_like(where),
                "glimpse": np.zeros_like(glimpse)} if best is None else best
    else:
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(J) & (np.isnan(best["J"]) | (J > best["J"]))
    best = {k: np.array(v) for k, v in best.items()}
    best["J"][take], best["iter"][take] = J[take], iter
    for k, src in (("what", what), ("where", where), ("glimpse", glimpse)):
        best[k][:, take] = src[:, take]

    out = {"J": J, "take": take, "best": best, "what": what, "where": where, "m_what": f(m_what), "v_what": f(v_what),
           "m_where": f(m_where), "v_where": f(v_where)}
    if not do_update:
        return out

    def adam(z, d, mu, sd, m, v, lr):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            g = d + (z - mu) / (sd * sd)
            m2 = beta1 * m + (1.0 - beta1) * g
            v2 = beta2 * v + (1.0 - beta2) * (g * g)
            z2 = z - lr * (m2 / c1) / (np.sqrt(v2 / c2) + eps)
        return z2, m2, v2

    z2, m2, v2 = adam(what, f(dwhat), w_loc, w_scale, out["m_what"], out["v_what"], float(lr_what))
    mk = mask[..., None]
    out["m_what"], out["v_what"] = np.where(mk, m2, out["m_what"]), np.where(mk, v2, out["v_what"])
    if float(lr_what) != 0.0:
        out["what"] = np.where(mk, z2, what)
    z2, m2, v2 = adam(where, f(dwhere), mu_where, sd_where, out["m_where"], out["v_where"], float(lr_where))
    out["m_where"], out["v_where"] = np.where(mk, m2, out["m_where"]), np.where(mk, v2, out["v_where"])
    if float(lr_where) != 0.0:
        g = float(guard_eps)
        if g > 0.0:                                                # |sx|, |sy| >= guard_eps: sign kept, +guard for 0
            s = z2[..., 0::2]
            z2[..., 0::2] = np.where(np.abs(s) < g, np.copysign(g, s), s)
        out["where"] = np.where(mk, z2, where)
    return out


class ParseRefiner(BoundStage):
    KIND = "refiner"
    ACCEPTS = ("scene", "particle")
    KEY_FIELDS = ("output_multiplier", "output_std", "guard_eps", "what_prior", "where_scale_prior", "where_shift_prior", "mfma_dtype")

    def __init__(self, parser, steps: int, lr_what: float, lr_where: float, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8):
        self._start = self.bind(parser)
        cfg = parser.engine.cfg
        check_arguments(cfg, steps, lr_what, lr_where, beta1, beta2, eps)
        import torch
        from . import hip as H
        self.parser, self.engine = parser, parser.engine
        self._bound = parser
        self.steps, self.lr_what, self.lr_where = int(steps), float(lr_what), float(lr_where)
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.T, self.R = parser.T, parser.R
        self.mask_threshold = parser.mask_threshold
        eng, dev = self.engine, self.engine.device
        T, B, A, N = self.T, self.R, int(cfg.n_appearance), self.steps
        (Hi, Wi), hw, P = cfg.img_size, cfg.n_crop, cfg.n_pix
        self.n_bands = int(H.lib().air_canvas_unroll_bands(B, int(Hi)))
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        with torch.cuda.device(dev):
            self.what, self.where = z((T, B, A)), z((T, B, 4))
            self.where_loc = self._start["where_loc"] if self._start["where_loc"] is not None else z((T, B, 4))
            # the Adam moments, one flat buffer (one fill): the where-shaped ones first, so that all four start 16-byte aligned
            self.moments = z((2 * T * B * 4 + 2 * T * B * A,))
            self.m_where, self.v_where = self.moments[:T * B * 4].view(T, B, 4), self.moments[T * B * 4:2 * T * B * 4].view(T, B, 4)
            self.m_what = self.moments[2 * T * B * 4:2 * T * B * 4 + T * B * A].view(T, B, A)
            self.v_what = self.moments[2 * T * B * 4 + T * B * A:].view(T, B, A)
            self.shapes = eng.gd.shapes
            self.act = [z((T * B, n)) for _, n in self.shapes]     # the decoder's activations; the last one = this iteration's glimpses
            self.g = [z((T * B, n)) for _, n in self.shapes]       # gradients at the layers' pre-activations (g[-1] = dglimpse)
            self.final_canvas, self.rec_parts = z((B, P)), z((self.n_bands, B))
            self.grad_what, self.grad_where = z((T, B, A)), z((T, B, 4))
            self.best_J, self.best_iter = z((B,), torch.float64), z((B,), torch.int32)
            self.best_what, self.best_where, self.best_glimpse = z((T, B, A)), z((T, B, 4)), z((T, B, hw))
            self.J_trace = z((N + 1, B))
        # the read-out of the best rows (what the parsers keep)
        self._ro = ReadOut(H, eng, T, B, A, cfg.img_size, self.n_bands, self.mask_threshold)
        self._ro.alias(self, rec_parts="rec_parts_out")
        self._H = H
        self._rebuild()
        eng.synchronize()

    def rows(self):
        """the provider protocol (stage.py): the best rows; presence_prob and the images are the start parse's"""
        st = self._start
        return {"what": self.best_what, "where": self.best_where, "glimpse": self.best_glimpse, "presence_prob": st["presence_prob"],
                "obs": st["obs"], "where_loc": self.where_loc, "gather_loc": False, "compacted": False}

    # ---- the launches behind the parser's own call ---------------------------------------------------------------------------
    def _build_plan(self):
        H, eng, par, st = self._H, self.engine, self.parser, self._start
        cfg = eng.cfg
        check_arguments(cfg, self.steps, self.lr_what, self.lr_where, self.beta1, self.beta2, self.eps)
        L, p, size = H.lib(), H._p, ctypes.c_size_t
        T, B, A, N = self.T, self.R, int(cfg.n_appearance), self.steps
        M, nl = T * B, len(self.shapes)
        (Hi, Wi), (hc, wc) = cfg.img_size, cfg.crop_size
        mult, std = float(cfg.output_multiplier), float(cfg.output_std)
        priors = prior_arguments(cfg)
        w, b = eng.gd.w, eng.gd.b
        plan = [(L.air_tile_rows, (p(st["what"]), p(self.what), 1, M * A), "air_tile_rows"),
                (L.air_tile_rows, (p(st["where"]), p(self.where), 1, M * 4), "air_tile_rows"),
                (L.air_fill, (p(self.moments), size(self.moments.numel()), 0.0), "air_fill")]
        for i in range(N + 1):
            if i > 0 or N > 0:
                x = self.what
                for j, (k, n) in enumerate(self.shapes):           # ELU on the hidden layers, none on the last (modules.py:86-91)
                    plan.append((L.air_linear_fwd, (p(x), p(w[j]), p(b[j]), p(self.act[j]), M, k, n,
                                                    H.ACT_NONE if j == nl - 1 else H.ACT_ELU, None, size(0)), "air_linear_fwd"))
                    x = self.act[j]
            glimpse = st["glimpse"] if i == 0 else self.act[-1]    # iteration 0: the start parse as the parser left it
            plan.append((L.air_canvas_unroll_fwd_banded,
                         (p(glimpse), p(self.where), p(par.presence), p(st["obs"]), None, p(self.final_canvas), p(self.rec_parts),
                          self.n_bands, T, B, Hi, Wi, hc, wc, mult, std), "air_canvas_unroll_fwd_banded"))
            update = i < N
            if update:
                plan.append((L.air_canvas_unroll_bwd,
                             (p(glimpse), p(self.where), p(par.presence), p(st["obs"]), p(self.final_canvas), p(self.g[-1]),
                              p(self.grad_where), T, B, Hi, Wi, hc, wc, mult, std, 1.0), "air_canvas_unroll_bwd"))
                for j in range(nl - 1, -1, -1):                    # dx_j = g_j . w_j^T, times elu'(act_{j-1}) on the hidden layers
                    k, n = self.shapes[j]
                    out = self.g[j - 1] if j > 0 else self.grad_what
                    plan.append((L.air_gemm, (0, 1, M, k, n, p(self.g[j]), n, p(w[j]), n, p(out), k, None,
                                              H.EPI_MUL_DELU if j > 0 else H.EPI_NONE, p(self.act[j - 1]) if j > 0 else None,
                                              k if j > 0 else 0, 0.0, None, None, size(0)), "air_gemm"))
            c1, c2 = 1.0 - self.beta1 ** (i + 1), 1.0 - self.beta2 ** (i + 1)
            opt = (p(self.grad_what), p(self.grad_where), p(self.m_what), p(self.v_what), p(self.m_where), p(self.v_where))
            plan.append((L.air_refine_step,
                         (p(self.what), p(self.where), p(glimpse), p(par.presence), p(self.rec_parts), self.n_bands,
                          opt[0] if update else None, opt[1] if update else None, p(self.where_loc), *priors,
                          *(opt[2:] if update else (None,) * 4), self.lr_what, self.lr_where, self.beta1, self.beta2, self.eps,
                          c1, c2, float(cfg.guard_eps), i, 1 if update else 0, T, B, A, hc * wc, p(self.best_J), p(self.best_iter),
                          p(self.best_what), p(self.best_where), p(self.best_glimpse), p(self.J_trace)), "air_refine_step"))
        self._plan = plan + [self._ro.objects(st["presence_prob"], par.num_objects, self.best_where, self.best_what)] + \
            self._ro.tail(self.best_glimpse, self.best_where, st["obs"])

    def launch_count(self) -> Dict[str, int]:
        """entries of one `parse()` call behind the bound parser's own (`parser` holds that parser's launch_count())"""
        N, nl = self.steps, len(self.shapes)
        return {"parser": self.parser.launch_count(), "start": 3, "decoder_fwd": nl * (N + 1 if N > 0 else 0), "canvas_fwd": N + 1,
                "canvas_bwd": N, "decoder_dx": nl * N, "refine_step": N + 1, "parse_objects": 1, "parse_render": 1, "rec_sum": 1}

    # ---- the parse ----------------------------------------------------------------------------------------------------------
    def parse(self, obs, *args, **kwargs):
        """The bound parser's `parse(obs, ...)` (further arguments go to it unchanged), then the refinement.  Returns device tensors
        that the NEXT call overwrites: every key of the parser's result -- num_objects, count_prob, presence, score, boxes, what, where,
        glimpse, the object table, reconstruction, rec, owner, area now describe the refined parse; presence_prob,
        num_steps_posterior and a ParticleParser's own read-outs are the parser's -- and
          objective [B] float64 (the best J), objective_start [B] (J of the start parse), best_iter [B] int32,
          objective_trace [steps+1, B] (the fp32 roundings of every iteration's J), grad_what [T, B, A], grad_where [T, B, 4]
          (d sum_b rec_b / d latents at iteration steps-1: without the prior terms; zeros when steps = 0).
        Same stream contract as the parsers."""
        eng = self.engine
        self._refresh_plan()
        base = self.parser.parse(obs, *args, **kwargs)
        self.check_parse(base, "refiner")
        self.gather_where_loc()
        eng._replay_or_run(self._graph, self._plan)
        eng.wait_for_engine()
        out = dict(base)
        out.update(self._ro.result(self.best_glimpse))
        out.update({"what": self.best_what, "where": self.best_where, "objective": self.best_J, "objective_start": self.J_trace[0],
                    "best_iter": self.best_iter, "objective_trace": self.J_trace, "grad_what": self.grad_what,
                    "grad_where": self.grad_where})
        out.pop("layers", None)                                    # (the parser's layers are the start parse's)
        return out
