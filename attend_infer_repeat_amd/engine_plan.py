"""Plan construction of the fused engine (engine.AIREngine): the train step as fixed lists of C-ABI launches over the engine's
buffers -- forward, hand-derived backward, optimiser, the fusions and riders of each regime.

Where each policy lives:
  this module        `PlanMixin._build_plans` is the driver: it reads top to bottom as the step does.  `_PlanBuilder` holds one build --
                     the regime decisions (latency / throughput, fp32 / bf16 data path, the AIR_* switches), one method per phase of
                     the step, and the values that cross phases as attributes set by the phase that decides them.
                     `_fold_closing_update` folds the closing update into the last backward launches.
  gemm_groups.py     which GEMM problems share a launch (chunks of 8, the long-K split, the wide / odd split, the split-K single
                     entry), the packing of the deferred weight gradients, and the Python mirror of the library's eligibility rules
                     (gemm_kernels.hip wide_group_eligible, wide_regime_weight_gradients, shortk_eligible).  Host arithmetic, tested
                     without a device.
  engine_mirrors.py  the bf16 mirrors of the throughput regime's bf16 data path and the dX-chain pass (AIR_DX_CHAIN=1).
  plan_describe.py   `describe_plans`: every plan as text, pointers by tensor name (the builder's regression record).
  launch.py          issuing a launch list: eager with roctx ranges, captured into a hipGraph, replayed.
engine.py keeps memory, capture / replay, the public API, the feeder and checkpoints."""
import ctypes
import os

import torch

from . import _lib
from . import gemm_groups as G
from . import hip as H
from .engine_config import _Mlp
from .plan_describe import describe_plans  # noqa: F401 (the read-out belongs next to the builder)

NONE, BIAS, BELU, MDELU, ADDAUX, ADDAUX_ELU = H.EPI_NONE, H.EPI_BIAS, H.EPI_BIAS_ELU, H.EPI_MUL_DELU, H.EPI_ADD_AUX, H.EPI_ADD_AUX_ELU
p, _env, _size = H._p, os.environ.get, ctypes.c_size_t
LSTM0 = "the first LSTM step"      # marks its place in _PlanBuilder.inserts


def _dp(t):
    return t.data_ptr() if t is not None else None


class _PlanBuilder:
    """One build of the plans of engine `e`.  The constructor takes every regime decision that needs nothing but the configuration;
    the phases, called by `PlanMixin._build_plans` in step order, append to `fwd` / `bwd` and leave what later phases need as
    attributes.  It launches nothing and allocates nothing but through `allocate()`."""

    def __init__(self, e):
        self.e, self.L, self.cfg = e, H.lib(), e.cfg
        cfg = e.cfg
        if cfg.mfma_dtype not in ("f32", "bf16"):
            raise ValueError("mfma_dtype must be 'f32' or 'bf16', got %r" % (cfg.mfma_dtype,))
        self.B, self.T, self.M = e.B, e.T, e.M
        self.Hd, self.A, self.P, self.hw = cfg.n_hidden, cfg.n_appearance, cfg.n_pix, cfg.n_crop
        (self.Hi, self.Wi), (self.hc, self.wc) = cfg.img_size, cfg.crop_size
        B, T, M, Hd, P = self.B, self.T, self.M, self.Hd, self.P
        self.prec = 1 if cfg.mfma_dtype == "bf16" else 0
        self.fwd, self.bwd, self.deferred_dw = [], [], []
        self.inserts = []             # (position in fwd, entry): the first LSTM step (LSTM0, built per variant) / entries only forward() gets
        # Throughput regime (thousands of rows): the weight gradients (K = rows, tiny outputs) leave the dX chain and are
        # formed at the end of the backward in a few launches of their own -- nothing but the optimiser consumes them, and a
        # launch that holds ALL of them has hundreds of 64x64 tiles: enough to fill the chip with the wide-tile kernel (16-byte
        # operand loads, 8 waves split K inside the workgroup) instead of ~11 launches of 16x16 tiles with 16-way K splits.
        self.throughput = self.defer_dw = M >= int(_env("AIR_DEFER_DW_MIN_ROWS", "768"))
        # bf16 DATA path (throughput regime of mfma_dtype="bf16"): the dense products read bf16 mirrors of their operands -- a
        # shadow of the flat parameter buffer kept by the optimiser launch, mirrors of the activations / gradients that GEMM
        # epilogues produce, the observation batch converted at the start of the step -- see _apply_bf16_mirrors
        self.use16 = self.prec == 1 and self.throughput and _env("AIR_BF16_STORAGE", "1") == "1"
        self.m16 = e._mirror_ptr if self.use16 else (lambda t: None)
        # priors left at None (model.py:174-209: that KL term is simply not added): the kernels still evaluate the rows against a
        # standard normal, but they enter neither the loss nor any gradient (weights 0 / pointers NULL below)
        self.has_what = cfg.what_prior is not None
        self.has_where = cfg.where_scale_prior is not None and cfg.where_shift_prior is not None
        self.analytic = bool(cfg.nsp_analytic)
        # continuous steps (cell.py:150-151): the entry points that draw the presence take no uniform variates and write the probability
        # itself; the canvas write's backward returns d/d presence, which joins d/d presence_prob in the steps-logit backward
        self.discrete = bool(cfg.discrete_steps)
        self.anneal = {None: 0, "exp": 1, "linear": 2}[cfg.nsp_anneal]
        self.pw, self.inv_b = (1.0 if cfg.use_prior else 0.0), 1.0 / B
        self.tail_mult = cfg.baseline_lr_mult if cfg.use_reinforce else 0.0
        self.n_norm, self.n_uni = e.noise_normal.numel(), e.u_pres.numel()
        self.rng_inc = (self.n_norm + 3) // 4 + (self.n_uni + 3) // 4
        # The two products over the P pixels of obs -- cell.py:125 (hoisted out of the time loop) + the obs columns of the baseline's
        # first layer (modules.py:131-143) -- have K = P (2500 / 10000) on B/16 x 16 tiles each: 128 workgroups, each
        # pulling its whole K range through ONE CU -- ingest-bound at half of the chip.  In the latency regime K is split in two
        # (4 problems, 256 workgroups, same launch) and the CONSUMERS add the halves where they read them: the next layer's
        # A-operand prologue forms elu(slab0 + slab1 + bias) (and stores it for the backward); the baseline's second half is
        # written straight into the buffer its second stage accumulates into (beta = 1) next to aux = first half.  No
        # cross-workgroup hand-off, no extra launch, fixed summation order.
        self.E0 = E0 = e.enc.shapes[0][1]
        lvl0_tiles = ((B + 15) // 16) * ((E0 + 15) // 16)
        # (the consumer -- the product over the E0 columns of the first hidden layer -- runs on the A-prologue kernel, which the
        #  library only has on 16x16 tiles: its launch must stay below the 1536-tile switch to 32x32 tiles)
        n_after = e.enc.shapes[1][1] if e.enc.n > 1 else 4 * Hd
        self.split0 = (lvl0_tiles * (2 if cfg.use_reinforce else 1) <= 128 and P >= 2048 and P % 4 == 0 and E0 % 16 == 0
                       and ((B + 15) // 16) * ((n_after + 15) // 16) <= 1536 and _env("AIR_SPLIT_K0", "1") == "1"
                       # (not on the bf16 data path -- many steps at a small batch, e.g. B = 64, T = 12: the consumer's A-prologue has no
                       #  bf16-mirror form and the first layer's activation would be a mirrored buffer no epilogue writes)
                       and not self.use16)
        self.E = e.enc.shapes[-1][1]
        lstm_tiles = ((B + 15) // 16) * ((Hd + 15) // 16)
        # In the latency regime the hoisted product gx = enc_out . W_x + b has no launch of its own -- the first LSTM step,
        # whose recurrent operand is the one-row initial state, accumulates it next to h0 . W_h and writes gx for the later steps
        # (air_lstm_first_step_fwd: same sums, same order, one dependent launch fewer).  Not when the first encoder layer is the
        # only one (its K-split halves are reduced by the gx product's A-prologue) and not beyond the fused-step tile count.
        # (latency regime only: in the throughput regime the gx product keeps its wide-tile launch)
        # ... and not where the gx product alone would leave the 4-wave 16x16 body (a batch of 256 or more at Hd = 256: the wide-tile
        # kernels), whose K order the first step repeats: the launch declines those shapes (gemm_groups.first_step_fits).
        self.fold_gx = (e.enc.n > 1 and not self.throughput and lstm_tiles <= int(_env("AIR_FUSE_LSTM_TILES", "512"))
                        and G.first_step_fits(B, Hd, self.E, int(_env("AIR_GEMM_WIDE_MIN_TILES", "1000")))
                        and _env("AIR_FOLD_GX", "1") == "1")
        # Recurrent product + gate math in ONE launch per step while the chain is latency bound (it is the only truly
        # sequential part of the step); at large batch the 32x32-tile GEMM + a pointwise pass re-reads less (measured:
        # B=1024 0.938 vs 0.954 ms/step), so the pair is kept there.
        self.fuse_lstm = lstm_tiles <= int(_env("AIR_FUSE_LSTM_TILES", "512"))
        # forward: beyond 512 tiles the library's wide-tile form of the fused step (16 rows x 64 units x 4 gates per workgroup)
        self.fuse_lstm_fwd = self.fuse_lstm or (Hd % 64 == 0 and self.E % 4 == 0 and _env("AIR_FUSE_LSTM_WIDE", "1") == "1")
        # (the step prologue rides in the first fused step only in the latency regime: the wide-tile form holds 133 KB of LDS
        #  per workgroup, so riding prologue workgroups would wait for a free CU -- 14.4 us against 8.5 + 4.9 for two launches)
        self.prologue_rides = self.fuse_lstm
        self.lstm16 = self.use16 and self.fuse_lstm_fwd and not self.fuse_lstm and e._lstm16_ok()
        # "attend" fusion: output layers of the transform / steps MLPs + where sampling + presence / num-steps + the glimpse
        # read in ONE launch (three dependent launches otherwise).  Needs a 16-byte addressable image that fits the
        # register-prefetch staging, and (backward) one workgroup per glimpse.
        self.fuse_attend = (P % 4 == 0) and (P // 4 <= 3 * 1024) and T <= 28 and M <= int(_env("AIR_FUSE_ATTEND_M", str(1 << 30)))
        # Latency regime with REINFORCE: the whole `what` head -- the product q = ge_out . W + b, the sampling with its KL
        # terms and the latent columns of the baseline input -- is ONE launch (air_what_head_fwd: a tile holds both halves of its
        # (row, latent dim) pairs) instead of a GEMM launch + air_what_sample_pack.  The KL row of a sample spans several tiles: the
        # tiles leave shares, the backward launch of the same head (air_gauss_sample_bwd*) adds them; a forward() on its own -- an
        # evaluation pass -- adds them with a small launch of its own, which the train step drops.
        self.what_head = (cfg.use_reinforce and self.analytic and self.discrete and not self.throughput
                          and _env("AIR_FUSE_WHAT_HEAD", "1") == "1")
        self.wp = cfg.what_prior if self.has_what else (0.0, 1.0)
        sp, shp = (cfg.where_scale_prior, cfg.where_shift_prior) if self.has_where else ((0.0, 1.0), (0.0, 1.0))
        if shp[0] is None:                  # a shift prior without `loc` is centred on the posterior's own mean (model.py:203-207):
            shp = (float("nan"), shp[1])    # the kernels' NaN convention (include/air_hip.h, air_gauss_sample_fwd)
        self.sp, self.shp = sp, shp
        self.eps = -1.0 if cfg.explore_eps is None else float(cfg.explore_eps)
        self.marks, self.rider_hosts = [], []
        self.pre_fwd, self.cvt_in_prologue, self.opening = [], False, None

    def allocate(self):
        """the lazily allocated buffers this build's decisions ask for and the EMA block, in the order earlier builds made them"""
        e, cfg, B, T, M = self.e, self.cfg, self.B, self.T, self.M
        if self.split0:
            self.slabs = e._buf("enc_slab0", (B, self.E0)), e._buf("enc_slab1", (B, self.E0))
        if not self.fuse_lstm_fwd:
            e.gates = e._buf("gates", (T, B, 4 * self.Hd))
        e.dpres = None if self.discrete else e._buf("dpres", (T, B))
        self.kl_parts_args = (None, 0, None)
        if self.what_head:
            n_kl = int(self.L.air_what_head_parts(self.A))
            e.kl_what_parts = e._buf("kl_what_parts", (n_kl, M))
            self.kl_parts_args = (p(e.kl_what_parts), n_kl, p(e.kl_what_row))
        # decay_rate: the two moving averages + the rate + the update switch as one device block (air_nvil's `ema_dev`); evaluation
        # passes (forward() alone) read the averages without moving them
        self.ema_p = None
        if cfg.decay_rate is not None and cfg.use_reinforce:
            if getattr(e, "ema_dev", None) is None:
                e.ema_dev = torch.tensor([0.0, 1.0, float(cfg.decay_rate), 1.0], dtype=torch.float32, device=e.device)
            e._fill_in(e.ema_dev[2:3], float(cfg.decay_rate))
            self.ema_p = p(e.ema_dev)
        if cfg.use_reinforce and not self.analytic:
            e.imp = e._buf("imp", (B,))

    # ---- descriptors and grouped launches --------------------------------------------------------------------------------------
    def desc(self, ta, tb, Mm, Nn, Kk, Aa, lda, Bb, ldb, Cc, ldc, bias=None, epi=NONE, aux=None, ldaux=0, beta=0.0,
             colsum=None, A2=None, a_bias=None, a_elu=0, a_out=None):
        return _lib.AirGemmDesc(int(ta), int(tb), Mm, Nn, Kk, _dp(Aa), lda, _dp(Bb), ldb, _dp(Cc), ldc, _dp(bias), epi,
                                _dp(aux), ldaux, float(beta), _dp(colsum), self.prec, _dp(A2), _dp(a_bias), int(a_elu),
                                _dp(a_out))

    def groups(self, plan, descs, allow_splitk=False):
        """[(kind, problems)] that dispatch `descs` (gemm_groups.plan_launch); in the throughput regime the weight gradients of the
        backward are set aside for `deferred_dw_phase` first"""
        if self.defer_dw and plan is self.bwd:
            self.deferred_dw.extend(d for d in descs if G.is_weight_gradient(d))
            descs = [d for d in descs if not G.is_weight_gradient(d)]
            if not descs:
                return []
        return G.plan_launch(descs, self.throughput, self.use16, allow_splitk)

    def grouped_array(self, descs):
        arr = (_lib.AirGemmDesc * len(descs))(*descs)
        self.e._keep.append(arr)
        return arr

    def emit(self, plan, kind, descs):
        L = self.L
        if kind == G.SPLITK:
            d = descs[0]
            plan.append((L.air_gemm_bf16 if self.prec else L.air_gemm,
                         (d.ta, d.tb, d.M, d.N, d.K, d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.bias, d.epilogue, d.aux, d.ldaux, d.beta,
                          d.colsum, p(self.e.ws), _size(self.e.ws.numel() * 4)), "air_gemm"))
        else:
            plan.append((L.air_gemm_grouped, (self.grouped_array(descs), len(descs)), "air_gemm_grouped"))

    def launch(self, plan, descs, allow_splitk=False):
        """one dispatch for all `descs` (a lone long-K problem may use the split-K single-GEMM entry instead)"""
        for kind, grp in self.groups(plan, descs, allow_splitk):
            self.emit(plan, kind, grp)

    def fwd_desc(self, m: _Mlp, i, x, ldx):
        k, n = m.shapes[i]
        last = i == m.n - 1
        xin, ld_in = (m.out[i - 1], m.shapes[i - 1][1]) if i > 0 else (x, ldx)
        return self.desc(0, 0, m.rows, n, k, xin, ld_in, m.w[i], n, m.out[i], n, bias=m.b[i],
                         epi=BIAS if (last and m.last_linear) else BELU)

    def mlp_fwd_multi(self, chains):
        """chains: [(mlp, x, ldx)] advanced level by level, one dispatch per level"""
        for i in range(max(m.n for m, _, _ in chains)):
            self.launch(self.fwd, [self.fwd_desc(m, i, x, ldx) for m, x, ldx in chains if i < m.n])

    def mlp_bwd_levels(self, chains, extra_first=(), extra_last=(), first_dx_done=False):
        """chains: dicts(m, x, ldx, g_last, dx_out=None, dx_aux=None).  g_last = gradient wrt the last layer's
        pre-activation.  Returns the problems of each dispatch: per level every chain's dW (+db) and dX.
        first_dx_done: the dX of every chain's LAST layer already exists (air_attend_bwd_dx); that level then only has
        weight gradients, which ride in the next level's dispatch."""
        desc = self.desc
        depth = max(c["m"].n for c in chains)
        gcur = {id(c["m"]): c["g_last"] for c in chains}
        carry, levels = [], []
        for s_ in range(depth):
            descs = carry
            carry = []
            for c in chains:
                m = c["m"]
                i = m.n - 1 - s_
                if i < 0:
                    continue
                k, n = m.shapes[i]
                g = gcur[id(m)]
                if i == 0 and "x_parts" in c:           # first layer fed by a concat: one dW problem per part
                    for j, (xp, ldp, k0, kn) in enumerate(c["x_parts"]):
                        descs.append(desc(1, 0, kn, n, m.rows, xp, ldp, g, n, m.dw[0][k0:k0 + kn], n,
                                          colsum=m.db[0] if j == 0 else None))
                    continue
                xin, ld_in = (m.out[i - 1], m.shapes[i - 1][1]) if i > 0 else (c["x"], c["ldx"])
                descs.append(desc(1, 0, k, n, m.rows, xin, ld_in, g, n, m.dw[i], n, colsum=m.db[i]))
                skip_dx = first_dx_done and i == m.n - 1
                if i > 0:
                    if not skip_dx:
                        descs.append(desc(0, 1, m.rows, k, n, g, n, m.w[i], n, m.g[i - 1], k, epi=MDELU,
                                          aux=m.out[i - 1], ldaux=k))
                    gcur[id(m)] = m.g[i - 1]
                elif c.get("dx_out") is not None and not skip_dx:
                    aux = c.get("dx_aux")
                    descs.append(desc(0, 1, m.rows, k, n, g, n, m.w[0], n, c["dx_out"], k,
                                      epi=MDELU if aux is not None else NONE, aux=aux, ldaux=k if aux is not None else 0))
            if s_ == 0:
                descs = list(extra_first) + descs
            if s_ == depth - 1:
                descs = descs + list(extra_last)
            if first_dx_done and s_ == 0 and depth > 1 and not extra_first:
                carry = descs                  # only weight gradients at this level: dispatch them with the next one
                continue
            levels.append(descs)
        return levels

    def mlp_bwd_multi(self, chains, **kw):
        for descs in self.mlp_bwd_levels(chains, **kw):
            self.launch(self.bwd, descs)

    # ---- argument tuples several entries share ---------------------------------------------------------------------------------
    def prologue_tail(self, with_noise):
        """what the step prologue takes wherever it runs: the noise to draw, the counters, the annealing schedule, the prior table
        and the tiled initial state it writes"""
        e, cfg = self.e, self.cfg
        return (p(e.noise_normal), _size(self.n_norm if with_noise else 0), p(e.u_pres), _size(self.n_uni if with_noise else 0),
                p(e.rng_state), p(e.step_dev), self.anneal, float(cfg.nsp_init), float(cfg.nsp_final), float(cfg.nsp_steps),
                float(cfg.nsp_hold_init), float(cfg.nsp_steps_div), p(e.prior_dev), self.T, p(e.h_seq[0]), p(e.c_seq[0]))

    def prologue(self, with_noise, cvt=False, gather=None):
        """the step prologue as a launch of its own; cvt: its extra workgroups convert the observation batch to its bf16 mirror
        (air_step_prologue_cvt); gather (an AirBatchGather, with cvt): they read the rows from the dataset instead and write both
        (air_step_prologue_gather_cvt)"""
        e, L = self.e, self.L
        tail = self.prologue_tail(with_noise)
        args = tail[:14] + (p(e.params["lstm/h0"]), p(e.params["lstm/c0"])) + tail[14:] + (self.B, self.Hd)
        obs16 = ctypes.c_void_p(e.obs16.data_ptr()) if cvt else None
        if gather is not None:
            return (L.air_step_prologue_gather_cvt, args + (ctypes.byref(gather), obs16), "air_step_prologue_gather_cvt")
        if cvt:
            return (L.air_step_prologue_cvt, args + (p(e.obs), obs16, _size(e.obs.numel())), "air_step_prologue_cvt")
        return (L.air_step_prologue, args, "air_step_prologue")

    def epilogue_args(self, n_model, n_total, gscale):
        """centred RMSProp over the first n_total elements of the flat buffers (two learning rates around n_model) + the counters"""
        e, cfg = self.e, self.cfg
        return (p(e.flat_params), p(e.flat_grads), p(e.flat_ms), p(e.flat_mg), p(e.flat_mom), _size(n_model), _size(n_total),
                p(e.lr_dev), self.tail_mult, cfg.rms_decay, cfg.rms_momentum, cfg.rms_eps, gscale, p(e.step_dev), p(e.rng_state),
                ctypes.c_uint64(self.rng_inc))

    def imp_weight(self, imp, dpres, dpres_scale):
        e, cfg = self.e, self.cfg
        return (self.L.air_imp_weight, (p(e.rec_parts), e.n_bands, p(e.rec), p(e.kl_n), float(cfg.nsp_weight),
                                        p(e.kl_what_row) if self.has_what else None, p(e.kl_where_row) if self.has_where else None,
                                        p(e.presence), self.T, self.B, imp, dpres, dpres_scale), "air_imp_weight")

    def batch_gather(self, copy_mask):
        e = self.e
        data, shuffle = e._feeder
        bg = _lib.AirBatchGather(data.data_ptr(), int(data.shape[0]), int(data.shape[1]), int(shuffle), self.B,
                                 e.feeder_seed.data_ptr(), e.step_dev.data_ptr(), e.obs.data_ptr(), e.batch_idx.data_ptr(), copy_mask)
        return bg

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def noise_plan(self):
        """noise only (used when forward() is asked to keep injected noise: the prologue then draws nothing)"""
        e = self.e
        return [(self.L.air_rng_fill, (p(e.noise_normal), _size(self.n_norm), p(e.u_pres), _size(self.n_uni), p(e.rng_state)),
                 "air_rng_fill")]

    def encoder_fwd(self):
        """the products over the pixels of obs (input encoder + the obs columns of the baseline's first layer) and the rest of the
        input encoder.  Leaves `enc_pro` (how consumers read the first layer's activation) and `opening` (the (obs column, K) pairs of
        the problems of the launch that opens the list, when that is a grouped launch: what the feeder may fold the gather into)."""
        e, cfg, desc, fwd = self.e, self.cfg, self.desc, self.fwd
        B, P, E0 = self.B, self.P, self.E0
        col = {}                                   # id(problem) -> first obs column it reads
        if self.split0:
            kh = (P // 2) // 16 * 16                       # both halves start 16-byte aligned (and on a chunk boundary)
            s0, s1 = self.slabs
            lvl0 = [desc(0, 0, B, E0, kh, e.obs, P, e.enc.w[0], E0, s0, E0),
                    desc(0, 0, B, E0, P - kh, e.obs[:, kh:], P, e.enc.w[0][kh:], E0, s1, E0)]
            if cfg.use_reinforce:
                n0 = e.bl.shapes[0][1]
                lvl0 += [desc(0, 0, B, n0, kh, e.obs, P, e.bl.w[0][:kh], n0, e.bl_obs, n0, bias=e.bl.b[0], epi=BIAS),
                         desc(0, 0, B, n0, P - kh, e.obs[:, kh:], P, e.bl.w[0][kh:P], n0, e.bl.out[0], n0)]
            col = {id(d): (kh if i % 2 else 0) for i, d in enumerate(lvl0)}
            launches = [self.groups(fwd, lvl0)]
            self.enc_pro = dict(A=s0, A2=s1, a_bias=e.enc.b[0], a_elu=1, a_out=e.enc.out[0])
        else:
            lvl0 = [self.fwd_desc(e.enc, 0, e.obs, P)]
            if cfg.use_reinforce:
                n0 = e.bl.shapes[0][1]
                lvl0.append(desc(0, 0, B, n0, P, e.obs, P, e.bl.w[0][:P], n0, e.bl_obs, n0, bias=e.bl.b[0], epi=BIAS))
            if ((B + 15) // 16) * ((max(d.N for d in lvl0) + 15) // 16) <= 256 or self.throughput:
                launches = [self.groups(fwd, lvl0)]     # few tiles: one launch, 16 waves per tile share the long K; throughput regime: one
                                                        # wide-tile launch for both products over obs (-2 % of the batch-1024 fp32 step)
            else:
                launches = [self.groups(fwd, [d], allow_splitk=True) for d in lvl0]
            self.enc_pro = None
        first = launches[0][0]
        if first[0] == G.GROUPED:
            self.opening = [(col.get(id(d), 0), d.K) for d in first[1]]
        for grps in launches:
            for kind, grp in grps:
                self.emit(fwd, kind, grp)
        if e.enc.n > 1:
            k1, n1 = e.enc.shapes[1]
            self.launch(fwd, [self.after_enc0(k1, n1, e.enc.w[1], n1, e.enc.out[1], e.enc.b[1], BELU)])
        for i in range(2, e.enc.n):
            self.launch(fwd, [self.fwd_desc(e.enc, i, None, 0)])

    def after_enc0(self, k, n, Bmat, ldb, Cc, bias, epi):
        """the product that consumes the first encoder layer's activation [B, E0]"""
        e, pro = self.e, self.enc_pro
        if pro is None:
            return self.desc(0, 0, self.B, n, k, e.enc.out[0], self.E0, Bmat, ldb, Cc, n, bias=bias, epi=epi)
        return self.desc(0, 0, self.B, n, k, pro["A"], self.E0, Bmat, ldb, Cc, n, bias=bias, epi=epi, A2=pro["A2"],
                         a_bias=pro["a_bias"], a_elu=pro["a_elu"], a_out=pro["a_out"])

    def lstm_fwd(self):
        """the hoisted product gx = enc_out . W_x + b and the T recurrences (cell.py:126-127).  With the fused steps the first one
        carries the step prologue: it is built per forward variant (`lstm_first_step`) and inserted at `lstm0_at`."""
        e, L, fwd, desc, m16 = self.e, self.L, self.fwd, self.desc, self.m16
        B, T, Hd, E = self.B, self.T, self.Hd, self.E
        enc_out = e.enc.out[-1]
        wg, bg = e.params["lstm/w_gates"], e.params["lstm/b_gates"]
        self.w_x, self.w_h = w_x, w_h = wg[:E], wg[E:]
        if self.fold_gx:
            pass
        elif e.enc.n == 1:
            self.launch(fwd, [self.after_enc0(E, 4 * Hd, w_x, 4 * Hd, e.gx, bg, BIAS)])
        else:
            self.launch(fwd, [desc(0, 0, B, 4 * Hd, E, enc_out, E, w_x, 4 * Hd, e.gx, 4 * Hd, bias=bg, epi=BIAS)])
        for t in range(T):
            if self.prologue_rides and t == 0:
                self.inserts.append((len(fwd), LSTM0))
            elif self.lstm16:
                # bf16 data path: W_h from the shadow, h_t from its mirror (h_0 = the tiled initial state has none)
                fwd.append((L.air_lstm_step_fwd_bf16, (p(e.h_seq[t]), m16(e.h_seq[t]), p(e.c_seq[t]), m16(w_h), 4 * Hd,
                                                       p(e.gx), 4 * Hd, p(e.h_seq[t + 1]), m16(e.h_seq[t + 1]),
                                                       p(e.c_seq[t + 1]), p(e.gate_act[t]), B, Hd, 1.0),
                            "air_lstm_step_fwd_bf16"))
            elif self.fuse_lstm_fwd:
                fwd.append((L.air_lstm_step_fwd, (p(e.h_seq[t]), p(e.c_seq[t]), p(w_h), 4 * Hd, p(e.gx), 4 * Hd,
                                                  p(e.h_seq[t + 1]), p(e.c_seq[t + 1]), p(e.gate_act[t]), B, Hd,
                                                  1.0, self.prec), "air_lstm_step_fwd"))
            else:
                self.launch(fwd, [desc(0, 0, B, 4 * Hd, Hd, e.h_seq[t], Hd, w_h, 4 * Hd, e.gates[t], 4 * Hd, epi=ADDAUX,
                                       aux=e.gx, ldaux=4 * Hd)])
                fwd.append((L.air_lstm_pointwise_fwd, (p(e.gates[t]), p(e.c_seq[t]), p(e.h_seq[t + 1]),
                                                       p(e.c_seq[t + 1]), p(e.gate_act[t]), B, Hd, 1.0),
                            "air_lstm_pointwise_fwd"))

    def lstm_first_step(self, with_noise):
        """the first fused LSTM step with the step prologue as extra workgroups; it reads h0 / c0 with a broadcast row stride (and,
        with the gx fold, forms gx on the way)"""
        e, L, Hd, E = self.e, self.L, self.Hd, self.E
        h0, c0 = p(e.params["lstm/h0"]), p(e.params["lstm/c0"])
        step = (p(self.w_h), 4 * Hd, p(e.gx), 4 * Hd, p(e.h_seq[1]), p(e.c_seq[1]), p(e.gate_act[0]), self.B, Hd, 1.0, self.prec)
        if self.fold_gx:
            return (L.air_lstm_first_step_fwd, (p(e.enc.out[-1]), E, E, p(self.w_x), p(e.params["lstm/b_gates"]), h0, c0) + step
                    + self.prologue_tail(with_noise), "air_lstm_first_step_fwd")
        return (L.air_lstm_step_fwd_prologue, (h0, c0) + step + self.prologue_tail(with_noise), "air_lstm_step_fwd_prologue")

    def attend_fwd(self):
        """transform / steps heads, where sampling, presence and the glimpse read (cell.py:129-151)"""
        e, L, cfg, fwd = self.e, self.L, self.cfg, self.fwd
        B, T, M, Hd, sp, shp = self.B, self.T, self.M, self.Hd, self.sp, self.shp
        h_all = self.h_all = e.h_seq[1:]                                                    # [T,B,Hd] contiguous
        u_p = p(e.u_pres) if self.discrete else None
        if self.fuse_attend:
            for i in range(max(e.tr.n, e.st.n) - 1):
                self.launch(fwd, [self.fwd_desc(m, i, h_all, Hd) for m in (e.tr, e.st) if i < m.n - 1])
            tr_in, tr_k = (e.tr.out[-2], e.tr.shapes[-1][0]) if e.tr.n > 1 else (h_all, Hd)
            st_in, st_k = (e.st.out[-2], e.st.shapes[-1][0]) if e.st.n > 1 else (h_all, Hd)
            fwd.append((L.air_attend_fwd, (p(tr_in), p(e.tr.w[-1]), p(e.tr.b[-1]), tr_k, p(st_in),
                                           p(e.st.w[-1]), p(e.st.b[-1]), st_k, p(e.tr.out[-1]),
                                           p(e.st.out[-1]), p(e.eps_where), cfg.transform_var_bias, sp[0], sp[1],
                                           shp[0], shp[1], p(e.where_loc), p(e.where_scale), p(e.where),
                                           p(e.kl_where_row), u_p, cfg.step_bias, self.eps, p(e.prior_dev),
                                           p(e.presence_prob), p(e.presence), p(e.q_n), p(e.kl_n),
                                           p(e.logp), p(e.step_w), p(e.obs), p(e.glimpse_in), T, B, self.Hi, self.Wi,
                                           self.hc, self.wc, self.prec, float(cfg.guard_eps)), "air_attend_fwd"))       # cell.py:129-151
        else:
            self.mlp_fwd_multi([(e.tr, h_all, Hd), (e.st, h_all, Hd)])                      # cell.py:129,138
            fwd.append((L.air_heads_fwd, (p(e.tr.out[-1]), 8, p(e.eps_where), cfg.transform_var_bias, 1,
                                          sp[0], sp[1], shp[0], shp[1], p(e.where_loc), p(e.where_scale),
                                          p(e.where), p(e.kl_where_row), M, 4,                # cell.py:129-133
                                          p(e.st.out[-1]), u_p, cfg.step_bias, self.eps, p(e.prior_dev),
                                          p(e.presence_prob), p(e.presence), p(e.q_n), p(e.kl_n), p(e.logp),
                                          p(e.step_w), T, B, float(cfg.guard_eps)), "air_heads_fwd"))                  # cell.py:137-151, prior.py
            fwd.append((L.air_st_read_fwd, (p(e.obs), p(e.where), p(e.glimpse_in), M, B, self.Hi, self.Wi, self.hc, self.wc),
                        "air_st_read_fwd"))                                                 # cell.py:135

    def what_fwd(self):
        """glimpse encoder (cell.py:153) and the `what` head (modules.py:20-21, cell.py:154-156); with the fused head the sum of its
        KL shares is an entry only evaluation passes get (the train step's backward of the head adds them)"""
        e, L, cfg, fwd, wp = self.e, self.L, self.cfg, self.fwd, self.wp
        B, T, M, A, Hd = self.B, self.T, self.M, self.A, self.Hd
        self.mlp_fwd_multi([(e.ge, e.glimpse_in, self.hw)])
        ge_out, G_ = e.ge.out[-1], e.ge.shapes[-1][1]
        if self.what_head:
            fwd.append((L.air_what_head_fwd, (p(ge_out), G_, G_, p(e.params["what/w"]), p(e.params["what/b"]), p(e.eps_what),
                                              cfg.what_scale_offset, wp[0], wp[1], p(e.q), p(e.what_loc), p(e.what_scale),
                                              p(e.what), p(e.kl_what_parts), A, p(e.where), p(e.presence),
                                              p(e.h_seq[T]), p(e.c_seq[T]), p(e.base_lat), T, B, Hd, Hd,
                                              float(cfg.guard_eps), self.prec), "air_what_head_fwd"))
            kl_sum = (L.air_sum_leading, (p(e.kl_what_parts), p(e.kl_what_row), self.kl_parts_args[1], _size(M)), "air_sum_leading")
            self.inserts.append((len(fwd), kl_sum))
        else:
            self.launch(fwd, [self.desc(0, 0, M, 2 * A, G_, ge_out, G_, e.params["what/w"], 2 * A, e.q, 2 * A,
                                        bias=e.params["what/b"], epi=BIAS)])
            if cfg.use_reinforce:
                # sample `what` + assemble the latent columns of the baseline input in one launch
                fwd.append((L.air_what_sample_pack, (p(e.q), 2 * A, p(e.eps_what), cfg.what_scale_offset, wp[0], wp[1],
                                                     p(e.what_loc), p(e.what_scale), p(e.what), p(e.kl_what_row),
                                                     A, p(e.where), p(e.presence), p(e.h_seq[T]), p(e.c_seq[T]),
                                                     p(e.base_lat), T, B, Hd, Hd, float(cfg.guard_eps)), "air_what_sample_pack"))
            else:
                fwd.append((L.air_gauss_sample_fwd, (p(e.q), 2 * A, p(e.eps_what), cfg.what_scale_offset, 0, wp[0],
                                                     wp[1], wp[0], wp[1], p(e.what_loc), p(e.what_scale), p(e.what),
                                                     p(e.kl_what_row), M, A, float(cfg.guard_eps)), "air_gauss_sample_fwd"))

    def decoder_baseline_fwd(self):
        """glimpse decoder (cell.py:158) next to the baseline's latent columns and later layers (model.py:218-259)"""
        e, cfg, fwd = self.e, self.cfg, self.fwd
        if not cfg.use_reinforce:
            self.mlp_fwd_multi([(e.gd, e.what, self.A)])
            return
        KL, n0 = cfg.baseline_in - self.P, e.bl.shapes[0][1]
        self.launch(fwd, [self.desc(0, 0, self.B, n0, KL, e.base_lat, KL, e.bl.w[0][self.P:], n0, e.bl.out[0], n0,
                                    epi=ADDAUX_ELU if e.bl.n > 1 or not e.bl.last_linear else ADDAUX,
                                    aux=e.bl_obs, ldaux=n0, beta=1.0 if self.split0 else 0.0),
                          self.fwd_desc(e.gd, 0, e.what, self.A)])
        for i in range(1, max(e.gd.n, e.bl.n)):
            self.launch(fwd, [self.fwd_desc(m, i, None, 0) for m in (e.gd, e.bl) if i < m.n])

    def canvas_fwd(self):
        """the canvas unroll (cell.py:159-165, model.py:319-324) and the tail of the objective.  NVIL (model.py:218-259): forward()
        alone finishes with it so that outputs() is complete (`fwd_tail`); a train step evaluates it as one extra workgroup of the
        canvas backward launch instead (independent work, one launch fewer).  Either way it is the consumer that adds the per-band
        shares of rec_loss_per_sample (and stores the sum in e.rec)."""
        e, L, cfg, B, NB = self.e, self.L, self.cfg, self.B, self.e.n_bands
        decoded = e.gd.out[-1]
        self.canvas_at = len(self.fwd)
        self.fwd.append((L.air_canvas_unroll_fwd_banded, (p(decoded), p(e.where), p(e.presence), p(e.obs),
                                                          p(e.canvas_steps), p(e.final_canvas), p(e.rec_parts), NB,
                                                          self.T, B, self.Hi, self.Wi, self.hc, self.wc, cfg.output_multiplier,
                                                          cfg.output_std), "air_canvas_unroll_fwd_banded"))
        ema_p = self.ema_p
        self.nvil_args = (p(e.rec_parts), NB, p(e.rec), p(e.bl.out[-1]), p(e.logp), p(e.nvil_out), p(e.dlogp), p(e.dbase))
        self.rec_sum = (L.air_sum_leading, (p(e.rec_parts), p(e.rec), NB, _size(B)), "air_sum_leading")
        self.nvil_parts = (L.air_nvil_parts, self.nvil_args + (B, ema_p), "air_nvil_parts")
        fwd_tail = [self.nvil_parts] if cfg.use_reinforce else [self.rec_sum]
        self.nvil_direct = None
        if cfg.use_reinforce and not self.analytic:
            # a non-analytic num-steps prior (model.py:157-163, 339-340): the step weights are the sampled presences and the prior's
            # per-sample value joins the importance weight -- formed by a small launch of its own, NVIL as the plain launch behind it
            self.nvil_direct = [self.imp_weight(p(e.imp), None, 0.0),
                                (L.air_nvil, (p(e.imp), p(e.bl.out[-1]), p(e.logp), p(e.nvil_out), p(e.dlogp), p(e.dbase),
                                              B, ema_p), "air_nvil")]
            fwd_tail = list(self.nvil_direct)
        if ema_p is not None:               # (forward() is an evaluation pass: the update switch is off around its NVIL launch)
            sw = ctypes.c_void_p(e.ema_dev.data_ptr() + 12)
            fwd_tail = [(L.air_fill, (sw, _size(1), 0.0), "air_fill")] + fwd_tail + [(L.air_fill, (sw, _size(1), 1.0), "air_fill")]
        self.fwd_tail = fwd_tail

    # ---- backward of opt_loss = mean(rec) + pw*(mean kl_n + mean sum_t w*(kl_what+kl_where)) + reinforce ----------------------------
    def canvas_bwd(self):
        """the canvas backward with NVIL, and the decision to fuse it with the canvas forward (`fuse_canvas`, `n_split`, `bl_levels`).
        Latency regime with REINFORCE: the canvas forward and the (recompute-form) backward are ONE launch -- the backward
        re-forms the canvas on each glimpse's footprint, so it reads nothing the forward writes (air_canvas_unroll_fwd_bwd) -- the
        train step's forward list then ends before the canvas; NVIL, which needs the forward's reconstruction shares, rides on
        the next pointwise launch (air_gauss_sample_bwd_nvil) and the baseline's backward, which needs NVIL, rides with the
        three launches after that (what / glimpse-encoder backward) instead of the decoder's.  35 -> 34 dependent launches.
        The two-role launch of the latency regime measured slower in the throughput regime (VALU bound chip-wide plus the
        recomputation: 0.594 against 0.580 ms at batch 1024)."""
        e, L, cfg, bwd = self.e, self.L, self.cfg, self.bwd
        B, T, M, P, NB = self.B, self.T, self.M, self.P, e.n_bands
        Hi, Wi, hc, wc, inv_b = self.Hi, self.Wi, self.hc, self.wc, self.inv_b
        # n_split: workgroups per backward unit of that launch (disjoint dglimpse rows, dwhere as n_split slabs that air_attend_bwd_dx
        # adds).  Measured (profiles/r04_canvas_split_ab.txt): with 2 the launch is FASTER only while it leaves CUs idle (batch 8:
        # 9.0 against 9.5 us); at batch 64 (192 units + 256 forward workgroups on 256 CUs) every workgroup repeats the unit's
        # staging and tables and the launch is slower (15.0 against 11.3 us; the step 0.2093 against 0.2070 ms): default 1 above
        # 128 glimpses, AIR_CANVAS_SPLIT overrides.
        n_split = int(_env("AIR_CANVAS_SPLIT", "2" if M <= 128 else "1")) if (self.fuse_attend and M * 2 + B * NB <= 1024) else 1
        n_split = max(1, min(4, n_split))
        fuse_canvas = (cfg.use_reinforce and self.analytic and self.discrete
                       and (not self.throughput or _env("AIR_FUSE_CANVAS_THROUGHPUT", "0") == "1")
                       # (the fused launch's backward re-forms the canvas from ALL T glimpses on each unit's footprint -- T^2 taps:
                       #  measured 0.2095 against 0.2111 ms per step at T = 3 (50x50 / 20x20), 0.3231 against 0.3194 ms at T = 5
                       #  (100x100 / 28x28; tools/runs/r04_x.sh): by default only up to T = 3; "1" / "0" force it on / off)
                       and (_env("AIR_FUSE_CANVAS", "auto") == "1" or (_env("AIR_FUSE_CANVAS", "auto") == "auto" and T <= 3))
                       # (what the library's launch takes: both grids at most 4096 workgroups, the LDS of both roles)
                       and L.air_canvas_unroll_fwd_bwd_fits(NB, n_split, T, B, Hi, Wi, hc, wc) == 1)
        self.bl_chain = dict(m=e.bl, g_last=e.dbase,
                             x_parts=[(e.obs, P, 0, P), (e.base_lat, cfg.baseline_in - P, P, cfg.baseline_in - P)])
        self.bl_levels = [[], [], []]
        if fuse_canvas:
            # the baseline's backward, level by level, to ride later launches -- one level per launch, in order: the `what`
            # backward, the glimpse encoder's first level, its last level
            lv = self.mlp_bwd_levels([self.bl_chain])
            if len(lv) > 1 + min(e.ge.n, 2):
                fuse_canvas = False                          # (a deeper baseline than there are launches to ride: the plain plan)
            else:
                lv = lv + [[]] * (3 - len(lv))
                self.bl_levels = [lv[0], lv[1], lv[2]] if e.ge.n >= 2 else [lv[0], lv[1], []]
        self.fuse_canvas, self.n_split = fuse_canvas, (n_split if fuse_canvas else 1)
        decoded, dpres_p = e.gd.out[-1], (None if self.discrete else p(e.dpres))
        cu_args = (p(decoded), p(e.where), p(e.presence), p(e.obs), p(e.final_canvas), p(e.gd.g[-1]),
                   p(e.dwhere_w), T, B, Hi, Wi, hc, wc, cfg.output_multiplier, cfg.output_std, inv_b)
        if fuse_canvas:
            bwd.append((L.air_canvas_unroll_fwd_bwd, (p(decoded), p(e.where), p(e.presence), p(e.obs),
                                                      p(e.canvas_steps), p(e.final_canvas), p(e.rec_parts), NB,
                                                      p(e.gd.g[-1]), p(e.dwhere_w), self.n_split, T, B, Hi, Wi, hc, wc,
                                                      cfg.output_multiplier, cfg.output_std, inv_b),
                        "air_canvas_unroll_fwd_bwd"))
        elif not self.discrete:
            # continuous steps: the canvas backward also returns d/d presence; a non-analytic prior weighs the KL rows with the presence
            # ITSELF (model.py:162-163), whose gradient -- the weighted rows -- is added behind it by the importance-weight launch
            bwd.append((L.air_canvas_unroll_bwd_dpresence, cu_args[:7] + (dpres_p,) + cu_args[7:], "air_canvas_unroll_bwd_dpresence"))
            if not self.analytic:
                bwd.append(self.imp_weight(p(e.imp) if cfg.use_reinforce else None, dpres_p, self.pw * inv_b))
                if cfg.use_reinforce:
                    bwd.append(self.nvil_direct[1])
            elif cfg.use_reinforce:
                bwd.append(self.nvil_parts)
            else:
                bwd.append(self.rec_sum)
        elif cfg.use_reinforce and self.nvil_direct is not None:
            bwd.extend(self.nvil_direct)
            bwd.append((L.air_canvas_unroll_bwd, cu_args, "air_canvas_unroll_bwd"))
        elif cfg.use_reinforce:
            bwd.append((L.air_canvas_unroll_bwd_nvil, cu_args + self.nvil_args + (self.ema_p,), "air_canvas_unroll_bwd_nvil"))
        else:
            bwd.append(self.rec_sum)          # nobody consumes rec in the step itself; keeps outputs() complete after train_step
            bwd.append((L.air_canvas_unroll_bwd, cu_args, "air_canvas_unroll_bwd"))

    def decoder_what_bwd(self):
        """decoder (+ baseline) backward, the backward of the `what` head and of the glimpse encoder.  Latency regime: the backward of
        the `what` head needs no launch of its own -- the decoder's first-layer dX IS its sample gradient, so the thread that finishes
        d_what[m, a] writes dq[m, a] and dq[m, A + a] in the same epilogue (air_gemm_grouped_gauss_bwd), and NVIL / the sum of the
        head's KL shares ride behind the tiles of that launch."""
        e, L, cfg, bwd, desc, wp = self.e, self.L, self.cfg, self.bwd, self.desc, self.wp
        B, M, A, pw, inv_b = self.B, self.M, self.A, self.pw, self.inv_b
        kl_scale = pw * inv_b if self.has_what else 0.0
        chains = [dict(m=e.gd, x=e.what, ldx=A, g_last=e.gd.g[-1], dx_out=e.d_what)]
        if cfg.use_reinforce and not self.fuse_canvas:                                      # model.py:253-259, 362-367
            chains.append(self.bl_chain)
        levels = self.mlp_bwd_levels(chains)
        for descs in levels[:-1]:
            self.launch(bwd, descs)
        closing = self.groups(bwd, levels[-1])
        for kind, grp in closing[:-1]:
            self.emit(bwd, kind, grp)
        self.fold_gauss_bwd = False
        if closing:
            kind, grp = closing[-1]
            which = [i for i, d in enumerate(grp) if d.C == e.d_what.data_ptr() and not d.ta and d.N == A and d.epilogue == NONE
                     and d.beta == 0.0 and not d.colsum]
            if (not self.throughput and self.analytic and self.discrete and _env("AIR_FUSE_GAUSS_BWD", "1") == "1"
                    and kind == G.GROUPED and sum(G.tiles16(d) for d in grp) <= 1000 and len(which) == 1):
                epi = _lib.AirGaussBwdEpi(which[0], _dp(e.q), 2 * A, _dp(e.eps_what), cfg.what_scale_offset, wp[0], wp[1],
                                          _dp(e.what_loc), _dp(e.what_scale), _dp(e._kl_weights), kl_scale, _dp(e.dq), 2 * A, A,
                                          float(cfg.guard_eps))
                e._keep.append(epi)
                nv = (self.nvil_args + (B, self.ema_p)) if self.fuse_canvas else (None, 0, None, None, None, None, None, None, 0, None)
                bwd.append((L.air_gemm_grouped_gauss_bwd, (self.grouped_array(grp), len(grp), ctypes.byref(epi)) + nv
                            + self.kl_parts_args + (M,), "air_gemm_grouped_gauss_bwd"))
                self.fold_gauss_bwd = True
            else:
                self.emit(bwd, kind, grp)
        if not self.fuse_canvas:
            self.marks.append((len(bwd), "glimpse_decoder/0/w"))   # gradients of [glimpse_decoder .. baseline] are final here
        gb_args = (p(e.q), 2 * A, p(e.eps_what), cfg.what_scale_offset, 0, wp[0], wp[1], wp[0], wp[1], p(e.what_loc),
                   p(e.what_scale), p(e.d_what), None, p(e._kl_weights), kl_scale, p(e.dq), 2 * A, M, A)
        if self.fold_gauss_bwd:
            pass
        elif self.fuse_canvas:
            bwd.append((L.air_gauss_sample_bwd_nvil, gb_args + self.nvil_args + (B, float(cfg.guard_eps), self.ema_p) + self.kl_parts_args,
                        "air_gauss_sample_bwd_nvil"))
        else:
            bwd.append((L.air_gauss_sample_bwd, gb_args + (float(cfg.guard_eps),) + self.kl_parts_args, "air_gauss_sample_bwd"))
        ge_out, G_ = e.ge.out[-1], e.ge.shapes[-1][1]
        self.launch(bwd, [desc(1, 0, G_, 2 * A, M, ge_out, G_, e.dq, 2 * A, e.grads["what/w"], 2 * A, colsum=e.grads["what/b"]),
                          desc(0, 1, M, G_, 2 * A, e.dq, 2 * A, e.params["what/w"], 2 * A, e.ge.g[-1], G_, epi=MDELU,
                               aux=ge_out, ldaux=G_)] + self.bl_levels[0])
        self.mlp_bwd_multi([dict(m=e.ge, x=e.glimpse_in, ldx=self.hw, g_last=e.ge.g[-1], dx_out=e.d_glimpse_in)],
                           extra_first=self.bl_levels[1], extra_last=self.bl_levels[2])
        self.marks.append((len(bwd), "glimpse_encoder/0/w"))       # + [glimpse_encoder, what] (+ decoder, baseline when fused)

    def attend_bwd(self):
        """glimpse read, where sampling and the presence / num-steps terms, then the transform / steps MLPs"""
        e, L, cfg, bwd = self.e, self.L, self.cfg, self.bwd
        B, T, M, Hd, sp, shp, pw, inv_b = self.B, self.T, self.M, self.Hd, self.sp, self.shp, self.pw, self.inv_b
        dlogp_p = p(e.dlogp) if cfg.use_reinforce else None
        dpres_p = None if self.discrete else p(e.dpres)
        # the gradient weights of the KL terms, shared by both forms
        kl_terms = (p(e.presence_prob), p(e.presence), p(e.prior_dev), pw * inv_b * float(cfg.nsp_weight),
                    p(e.kl_what_row) if self.has_what else None, p(e.kl_where_row) if self.has_where else None,
                    pw * inv_b if self.analytic else 0.0, dlogp_p, dpres_p)
        if self.fuse_attend:
            # ... including the dX of the two MLP output layers (K = 8 and 1): their launch disappears from the chain, their
            # dW / bias gradients join the next level's launch
            def last_dx(m, dx_top):
                if m.n > 1:
                    return p(m.out[-2]), p(m.g[-2]), m.shapes[-1][0], m.shapes[-1][0]
                return None, p(dx_top), Hd, Hd
            bwd.append((L.air_attend_bwd_dx, (p(e.obs), p(e.where), p(e.d_glimpse_in), p(e.dwhere_r),
                                              p(e.tr.out[-1]), p(e.eps_where), cfg.transform_var_bias, sp[0], sp[1],
                                              shp[0], shp[1], p(e.where_loc), p(e.where_scale), p(e.dwhere_w), self.n_split,
                                              p(e._kl_weights), pw * inv_b if self.has_where else 0.0, p(e.tr.g[-1])) + kl_terms
                        + (p(e.st.out[-1]), cfg.step_bias, self.eps, p(e.st.g[-1]), T, B, self.Hi, self.Wi, self.hc, self.wc,
                           p(e.tr.w[-1])) + last_dx(e.tr, e.dH) + (p(e.st.w[-1]),) + last_dx(e.st, e.dH_b)
                        + (self.prec, float(cfg.guard_eps)), "air_attend_bwd_dx"))
        else:
            bwd.append((L.air_st_read_bwd, (p(e.obs), p(e.where), p(e.d_glimpse_in), p(e.dwhere_r), None, M,
                                            B, self.Hi, self.Wi, self.hc, self.wc), "air_st_read_bwd"))
            bwd.append((L.air_heads_bwd, (p(e.tr.out[-1]), 8, p(e.eps_where), cfg.transform_var_bias, 1,
                                          sp[0], sp[1], shp[0], shp[1], p(e.where_loc), p(e.where_scale),
                                          p(e.dwhere_w), p(e.dwhere_r), p(e._kl_weights), pw * inv_b if self.has_where else 0.0,
                                          p(e.tr.g[-1]), 8, M, 4) + kl_terms
                        + (p(e.st.out[-1]), cfg.step_bias, self.eps, p(e.st.g[-1]), T, B, float(cfg.guard_eps)), "air_heads_bwd"))
        self.mlp_bwd_multi([dict(m=e.tr, x=self.h_all, ldx=Hd, g_last=e.tr.g[-1], dx_out=e.dH),
                            dict(m=e.st, x=self.h_all, ldx=Hd, g_last=e.st.g[-1], dx_out=e.dH_b)],
                           first_dx_done=self.fuse_attend)
        self.marks.append((len(bwd), "transform/0/w"))             # + [transform, steps]

    def bptt(self):
        """BPTT through the T recurrences (dgates_t . W_h^T accumulates into dH[t-1] with beta = 1).  Leaves `dgx` (the sum over
        time of dgates: what the hoisted x.W_x receives), `dc0` (the gradient of the initial cell state) and `rider_hosts`
        ((index in bwd, entry with an optimiser slice, its arguments, name): see `riders`)."""
        e, L, bwd, m16 = self.e, self.L, self.bwd, self.m16
        B, T, Hd, w_h = self.B, self.T, self.Hd, self.w_h
        self.dgx = e.dgx if T > 1 else e.dgates[0]
        fuse_bwd = self.fuse_lstm_fwd            # (the library picks the 16-wave or the wide-tile form of the link by size)
        lstm16 = self.lstm16
        # In the latency regime the entry of the BPTT -- the pointwise backward of step T-1, a launch of its own
        # whose only consumer is the link of step T-2 -- is formed inside that link (air_lstm_step_bwd_entry: every workgroup builds
        # its A operand dgates_{T-1} from the saved activations; one dependent launch fewer).  AIR_LSTM_BWD_ENTRY=0: the two launches.
        entry_fold = (self.fuse_lstm and fuse_bwd and not lstm16 and T >= 2 and self.prec == 0
                      and L.air_lstm_step_bwd_entry_fits(B, Hd) == 1 and _env("AIR_LSTM_BWD_ENTRY", "1") == "1")
        dc_in, dc_out = None, e.dc_a
        for t in reversed(range(T)):
            saved = (p(e.gate_act[t]), p(e.c_seq[t]), p(e.c_seq[t + 1]))
            acc = p(e.dgates[T - 1]) if t == T - 2 else p(e.dgx)      # what the running dgx adds this step's dgates to
            if entry_fold and t == T - 1:
                entry_dc = dc_out       # (step T-1's results go where the pointwise launch wrote them: dgates[T-1], dc_a)
            elif entry_fold and t == T - 2:
                ent_args = (p(e.gate_act[T - 1]), p(e.c_seq[T - 1]), p(e.c_seq[T]), p(e.dH[T - 1]), p(e.dH_b[T - 1]),
                            p(e.dgates[T - 1]), p(entry_dc), p(w_h), p(e.dH[t]), p(e.dH_b[t])) + saved + (
                            p(e.dgates[t]), p(dc_out), p(e.dgx), B, Hd)
                self.rider_hosts.append((len(bwd), L.air_lstm_step_bwd_entry, ent_args, "air_lstm_step_bwd_entry"))
                bwd.append((L.air_lstm_step_bwd_entry, ent_args + (None,), "air_lstm_step_bwd_entry"))
            elif lstm16 and t == T - 1:
                bwd.append((L.air_lstm_pointwise_bwd_bf16, saved + (p(e.dH[t]), p(e.dH_b[t]), None, p(e.dgates[t]),
                                                                    m16(e.dgates[t]), p(dc_out), B, Hd),
                            "air_lstm_pointwise_bwd_bf16"))
            elif lstm16:
                bwd.append((L.air_lstm_step_bwd_bf16, (p(e.dgates[t + 1]), m16(e.dgates[t + 1]), m16(w_h), p(e.dH[t]),
                                                       p(e.dH_b[t]), p(dc_in)) + saved + (acc, p(e.dgates[t]), m16(e.dgates[t]),
                                                       p(dc_out), p(e.dgx), m16(e.dgx), B, Hd), "air_lstm_step_bwd_bf16"))
            elif t == T - 1 or not fuse_bwd:
                pw_args = saved + (p(e.dH[t]), p(e.dH_b[t]), p(dc_in) if dc_in is not None else None, p(e.dgates[t]), p(dc_out), B, Hd)
                if self.fuse_lstm:
                    self.rider_hosts.append((len(bwd), L.air_lstm_pointwise_bwd_opt, pw_args, "air_lstm_pointwise_bwd_opt"))
                bwd.append((L.air_lstm_pointwise_bwd, pw_args, "air_lstm_pointwise_bwd"))
                if not fuse_bwd and t > 0:    # dgates_t . W_h^T accumulates into dH[t-1] (beta = 1)
                    self.launch(bwd, [self.desc(0, 1, B, Hd, 4 * Hd, e.dgates[t], 4 * Hd, w_h, 4 * Hd, e.dH[t - 1], Hd, beta=1.0)])
            else:
                # one BPTT link per launch: dgates_{t+1}.W_h^T + direct dh terms -> gate backward of step t -> running dgx
                link_args = (p(e.dgates[t + 1]), p(w_h), p(e.dH[t]), p(e.dH_b[t]), p(dc_in)) + saved + (
                             acc, p(e.dgates[t]), p(dc_out), p(e.dgx), B, Hd, self.prec)
                self.rider_hosts.append((len(bwd), L.air_lstm_step_bwd_opt, link_args, "air_lstm_step_bwd_opt"))
                bwd.append((L.air_lstm_step_bwd, link_args, "air_lstm_step_bwd"))
            dc_in, dc_out = dc_out, (e.dc_b if dc_out is e.dc_a else e.dc_a)      # the two cell-gradient buffers alternate
        if not fuse_bwd and T > 1:
            bwd.append((L.air_sum_leading, (p(e.dgates), p(e.dgx), T, _size(B * 4 * Hd)), "air_sum_leading"))
        self.dc0 = dc_in

    def encoder_bwd(self):
        """d h_{-1}, d enc_out, the input encoder's backward and the LSTM's weight gradients"""
        e, desc = self.e, self.desc
        B, T, M, Hd, E, P = self.B, self.T, self.M, self.Hd, self.E, self.P
        enc_out, gw, dgx = e.enc.out[-1], e.grads["lstm/w_gates"], self.dgx
        self.launch(self.bwd, [desc(0, 1, B, Hd, 4 * Hd, e.dgates[0], 4 * Hd, self.w_h, 4 * Hd, e.dh_init, Hd),   # d h_{-1}
                               desc(0, 1, B, E, 4 * Hd, dgx, 4 * Hd, self.w_x, 4 * Hd, e.enc.g[-1], E, epi=MDELU, aux=enc_out,
                                    ldaux=E)])                                                 # d enc_out (pre-activation)
        # dW_h (+ db_gates) and dW_x have no dependants before the optimiser: they ride along with the last launch of the
        # chain (the input encoder's first-layer dW, another wide throughput-type problem) instead of costing their own
        lstm_dw = [desc(1, 0, Hd, 4 * Hd, M, e.h_seq[:T], Hd, e.dgates, 4 * Hd, gw[E:], 4 * Hd,
                        colsum=e.grads["lstm/b_gates"]),                                     # dW_h, db_gates
                   desc(1, 0, E, 4 * Hd, B, enc_out, E, dgx, 4 * Hd, gw[:E], 4 * Hd)]        # dW_x
        lstm_tail = [desc(1, 0, 1, Hd, B, e.ones_b, 1, e.dh_init, Hd, e.grads["lstm/h0"], Hd),   # dh0
                     desc(1, 0, 1, Hd, B, e.ones_b, 1, self.dc0, Hd, e.grads["lstm/c0"], Hd)]    # dc0
        # In the latency regime the LSTM's weight gradients leave the LAST launch for the one in front of it (they
        # have been ready since the BPTT closed): the closing launch -- 19 us with the folded update of input encoder + LSTM --
        # then holds the input encoder's first layer only, and the LSTM's half of that update runs in the epilogue of a launch
        # that left most of the chip idle.  AIR_LSTM_DW_EARLY=0: the previous placement (A/B).
        self.lstm_dw_early = (not self.throughput and not self.use16 and e.enc.n >= 2 and _env("AIR_LSTM_DW_EARLY", "1") == "1")
        chain = [dict(m=e.enc, x=e.obs, ldx=P, g_last=e.enc.g[-1])]
        if self.lstm_dw_early:
            self.mlp_bwd_multi(chain, extra_first=lstm_tail + lstm_dw)
        else:
            self.mlp_bwd_multi(chain, extra_first=lstm_tail, extra_last=lstm_dw)

    def deferred_dw_phase(self):
        """throughput regime: the weight gradients set aside by `groups`, in a few launches at the end of the backward
        (gemm_groups.deferred_dw_groups)"""
        if not self.deferred_dw:
            return
        for grp in G.deferred_dw_groups(self.deferred_dw, self.prec != 0):
            self.emit(self.bwd, G.GROUPED, grp)
        self.marks = []                            # no gradient slice is final before the end of the backward

    def l2(self):
        """L2 term (model.py:346-353): g += l2 * w on the 2-D model variables, the last launch of the backward (so every protocol
        -- single GPU, data parallel: the all-reduced sum of `world` identical terms is scaled back by 1/world -- sees it).
        Rare switch (0 in the script): the riders / folded update, which consume gradients before the end, are then off."""
        e, cfg = self.e, self.cfg
        if not (cfg.l2_weight and cfg.l2_weight > 0.0):
            return
        spans = []
        for k, shape in e.param_shapes.items():
            if len(shape) == 2 and not k.startswith("baseline/"):
                lo = e.param_offsets[k]
                if spans and spans[-1][1] == lo:
                    spans[-1][1] = lo + e.param_sizes[k]
                else:
                    spans.append([lo, lo + e.param_sizes[k]])
        if len(spans) > 32:
            raise _lib.AirHipError("more than 32 separate 2-D model tensors: the L2 launch takes 32 slices")
        lo_arr = (ctypes.c_size_t * len(spans))(*[a for a, _ in spans])
        hi_arr = (ctypes.c_size_t * len(spans))(*[b_ for _, b_ in spans])
        e._keep += [lo_arr, hi_arr]
        self.bwd.append((self.L.air_l2_grad_add, (p(e.flat_grads), p(e.flat_params), lo_arr, hi_arr, len(spans), float(cfg.l2_weight)),
                         "air_l2_grad_add"))
        self.marks, self.rider_hosts = [], []

    # ---- bf16 data path, optimiser, assembly -----------------------------------------------------------------------------------------
    def bf16_data_path(self):
        """bf16 data path: the descriptors of both lists get their mirrors; the conversion of the observation batch opens the forward
        -- as extra workgroups of the step prologue when that is a launch of its own (air_step_prologue_cvt: the two independent
        tiny launches that opened the step are one), as a launch otherwise"""
        e = self.e
        e._apply_bf16_mirrors([self.fwd, self.bwd])
        e._dx_chain_launches = 0
        # (measured and not adopted: 0.47-0.50 against 0.415-0.425 ms per step at configs[4], profiles/r06_dx_chain_rejected.txt;
        #  AIR_DX_CHAIN=1 switches the pass on)
        if self.throughput and _env("AIR_DX_CHAIN", "0") == "1":
            self.bwd[:] = e._fuse_dx_chains(self.bwd)
        self.cvt_in_prologue = (not self.prologue_rides and _env("AIR_FUSE_PROLOGUE_CVT", "1") == "1" and e.obs.numel() % 4 == 0)
        if not self.cvt_in_prologue:
            self.pre_fwd = [(self.L.air_f32_to_bf16, (p(e.obs), ctypes.c_void_p(e.obs16.data_ptr()), _size(e.obs.numel())),
                             "air_f32_to_bf16")]

    def optimizer_factory(self):
        """gscale -> the update's entries: both centred-RMSProp updates + device counters in one launch"""
        e, L, cfg = self.e, self.L, self.cfg
        if not cfg.rms_centered:
            # tf.train.RMSPropOptimizer(centered=False) (model.py:265 with other opt_kwargs): the generic update kernel on the two
            # segments + the counters; no riders (the BPTT riders and the fold are the centred form)
            if self.use16:
                raise _lib.AirHipError("the bf16 data path keeps its parameter shadow in the centred update launch: centered=False is not available with it")
            tail_mult, rng_inc = self.tail_mult, self.rng_inc
            seg = lambda lo, hi, mult, gscale: (L.air_rmsprop, (
                ctypes.c_void_p(e.flat_params.data_ptr() + 4 * lo), ctypes.c_void_p(e.flat_grads.data_ptr() + 4 * lo),
                ctypes.c_void_p(e.flat_ms.data_ptr() + 4 * lo), ctypes.c_void_p(e.flat_mg.data_ptr() + 4 * lo),
                ctypes.c_void_p(e.flat_mom.data_ptr() + 4 * lo), _size(hi - lo), p(e.lr_dev), mult, cfg.rms_decay,
                cfg.rms_momentum, cfg.rms_eps, 0, gscale), "air_rmsprop")
            self.rider_hosts = []
            return lambda gscale: (
                [seg(0, e.n_model, 1.0, gscale)] + ([seg(e.n_model, e.n_total, tail_mult, gscale)] if e.n_total > e.n_model and tail_mult else [])
                + [(L.air_counter_add, (p(e.step_dev), ctypes.c_int64(1)), "air_counter_add"),
                   (L.air_rng_advance, (p(e.rng_state), ctypes.c_uint64(rng_inc)), "air_rng_advance")])
        if self.use16:
            shadow = p(e.flat_params16)
            return lambda gscale: [(L.air_step_epilogue_shadow, self.epilogue_args(e.n_model, e.n_total, gscale) + (shadow,),
                                    "air_step_epilogue_shadow")]
        return lambda gscale: [(L.air_step_epilogue, self.epilogue_args(e.n_model, e.n_total, gscale), "air_step_epilogue")]

    def forward_plan(self, with_noise, evaluation, gather=None):
        """one variant of the forward list.  The prologue is a launch of its own or -- with the fused LSTM steps -- part of the
        first LSTM step; evaluation (forward()): complete outputs -- the sum of the `what` head's KL shares, the canvas, `fwd_tail`;
        a train step leaves them to its backward (NVIL rides in the first backward launch, the head's backward adds the shares, and
        with `fuse_canvas` the canvas forward IS the first backward launch)."""
        body, at = [], 0
        for pos, entry in self.inserts:
            body += self.fwd[at:pos]
            if entry is LSTM0:
                body.append(self.lstm_first_step(with_noise))
            elif evaluation:
                body.append(entry)
            at = pos
        body += self.fwd[at:]
        if self.fuse_canvas and not evaluation:
            assert body[-1][2] == "air_canvas_unroll_fwd_banded" and self.canvas_at == len(self.fwd) - 1
            body = body[:-1]
        head = [] if self.prologue_rides else [self.prologue(with_noise, cvt=self.cvt_in_prologue, gather=gather)]
        return self.pre_fwd + head + body + (self.fwd_tail if evaluation else [])

    def train_forward_plan(self):
        """the forward of a train step; with a dataset attached (attach_dataset) the batch itself is drawn by its first launch: no
        host work between updates.  Sets e._fold_gather."""
        e, L, B, P = self.e, self.L, self.B, self.P
        if getattr(e, "_feeder", None) is None:
            return self.forward_plan(True, False)
        data, shuffle = e._feeder
        e._fold_gather = False
        fold_on = _env("AIR_FOLD_GATHER", "1") == "1"
        opens_with_products = self.prologue_rides and not self.pre_fwd and self.opening is not None
        if fold_on and opens_with_products:
            # When the step opens with the products over the pixels of obs (latency regime: the K-split halves of the input
            # encoder's and the baseline's first layers), the gather is folded into their A-operand load -- row m is read from item
            # idx_m of the dataset and the first column of tiles writes it to `obs` for every later reader -- instead of being a
            # dependent launch of its own (air_gemm_grouped_gather; AIR_FOLD_GATHER=0: the two launches).  Bit-identical either way:
            # the fits rule takes only groups air_gemm_grouped is sure to run on the gather's 16-wave K-split body (group_long_k below
            # the wide-tile regime: gemm_kernels.hip group_on_long_k_body).
            # the problems that write obs: one per distinct (column offset, K) -- together they must tile [0, P)
            seen, mask = {}, 0
            for i, key in enumerate(self.opening):
                if key not in seen:
                    seen[key] = i; mask |= 1 << i
            cover = sorted(seen)
            tiled = cover[0][0] == 0 and all(cover[j][0] + cover[j][1] == cover[j + 1][0] for j in range(len(cover) - 1)) \
                and cover[-1][0] + cover[-1][1] == P
            plan = self.forward_plan(True, False)
            arr, n_d = plan[0][1]
            bg = self.batch_gather(mask)
            if tiled and int(data.shape[1]) == P and L.air_gemm_grouped_gather_fits(arr, n_d, ctypes.byref(bg)) == 1:
                e._keep.append(bg)
                e._fold_gather = True
                return [(L.air_gemm_grouped_gather, (arr, n_d, ctypes.byref(bg)), "air_gemm_grouped_gather")] + plan[1:]
        if fold_on and self.cvt_in_prologue and int(data.shape[1]) == P and P % 4 == 0:
            # bf16 data path (throughput regime): the step opens with the prologue whose extra workgroups convert obs to its bf16
            # mirror -- they read the rows from the dataset instead and write both (air_step_prologue_gather_cvt): no gather launch
            bg = self.batch_gather(0)
            e._keep.append(bg)
            e._fold_gather = True
            return self.forward_plan(True, False, gather=bg)
        gather = (L.air_batch_gather, (p(data), ctypes.c_longlong(data.shape[0]), int(data.shape[1]),
                                       p(e.feeder_seed), p(e.step_dev), int(shuffle), p(e.obs), B,
                                       p(e.batch_idx)), "air_batch_gather")
        return [gather] + self.forward_plan(True, False)

    def grad_buckets(self):
        """data-parallel gradient buckets: (end index in the backward plan, [lo, hi) slice of the flat gradient buffer that
        is final once the plan has run up to that index); contiguous, from the tail of the buffer to its head"""
        e, out, hi = self.e, [], self.e.n_total
        for idx, first in self.marks:
            lo = e.param_offsets[first]
            out.append((idx, lo, hi)); hi = lo
        out.append((len(self.bwd), 0, hi))
        return out

    def riders(self):
        """Single-GPU train step in the latency regime: the centred-RMSProp update of everything whose gradient is final before
        the BPTT chain (all but the input encoder and the LSTM: half of the 94 MB the update streams) rides as extra
        workgroups of the BPTT launches -- 64 tiles each, three quarters of the chip idle -- and the closing launch only
        updates the head of the buffer.  backward() / data-parallel steps (update after the all-reduce) keep the plain plans.
        Returns (backward with riders, closing update, start of the riders' range) or None."""
        e, cfg, hosts = self.e, self.cfg, self.rider_hosts
        if not (hosts and self.marks and not self.defer_dw and _env("AIR_OPT_RIDERS", "1") == "1"):
            return None
        r_lo, r_hi = e.param_offsets[self.marks[-1][1]], e.n_total
        if not (r_lo % 4 == 0 and r_hi % 4 == 0 and e.n_model % 4 == 0 and r_lo > 0 and r_hi > r_lo):
            return None
        nh = len(hosts)
        cuts = [r_lo + ((r_hi - r_lo) * i // nh) // 4 * 4 for i in range(nh)] + [r_hi]
        riders = list(self.bwd)
        e._rider_slices = []
        for (idx, fn, args, name), lo, hi in zip(hosts, cuts[:-1], cuts[1:]):
            sl = _lib.AirRmspropSlice(_dp(e.flat_params), _dp(e.flat_grads), _dp(e.flat_ms), _dp(e.flat_mg),
                                      _dp(e.flat_mom), lo, hi, e.n_model, _dp(e.lr_dev), self.tail_mult,
                                      cfg.rms_decay, cfg.rms_momentum, cfg.rms_eps, 1.0)
            e._rider_slices.append(sl)
            e._keep.append(sl)
            riders[idx] = (fn, args + (ctypes.byref(sl),), name)
        rest = [(self.L.air_step_epilogue, self.epilogue_args(min(e.n_model, r_lo), r_lo, 1.0), "air_step_epilogue")]
        return riders, rest, r_lo


class PlanMixin:
    """`_build_plans` and the closing fold; mixed into AIREngine"""

    def _build_plans(self):
        """The step as a fixed list of C-ABI launches.  It is launch/latency bound at batch 64 (~6 us per dependent
        launch), so independent GEMMs are dispatched together (air_gemm_grouped: the dW / dX pair of a layer, the
        transform / steps heads, decoder + baseline levels) and the tiny ops are fused (step prologue / epilogue,
        presence + num-steps)."""
        self._keep = getattr(self, "_keep", [])     # whatever a plan entry of any build points to stays alive (graphs hold pointers)
        b = _PlanBuilder(self)
        self._defer_dw, self._use16, self._rng_inc = b.defer_dw, b.use16, b.rng_inc
        self._fold_gx, self._what_head = b.fold_gx, b.what_head
        self._kl_weights = self.step_w if b.analytic else self.presence       # model.py:157-163
        # side effects of a build, once each: the bf16 mirrors, the buffers this regime asks for and the EMA block ...
        if b.use16:
            self._alloc_bf16_mirrors()
        b.allocate()
        self._kl_parts_args = b.kl_parts_args
        self._plan_rng = b.noise_plan()
        # forward
        b.encoder_fwd()
        b.lstm_fwd()
        b.attend_fwd()
        b.what_fwd()
        b.decoder_baseline_fwd()
        b.canvas_fwd()
        # backward
        b.canvas_bwd()
        b.decoder_what_bwd()
        b.attend_bwd()
        b.bptt()
        b.encoder_bwd()
        b.deferred_dw_phase()
        b.l2()
        self._fold_gauss_bwd, self._lstm_dw_early = b.fold_gauss_bwd, b.lstm_dw_early
        if b.use16:
            b.bf16_data_path()
            self._sync_param_shadow()               # ... and the refresh of the parameter shadow (a launch on the engine's stream)
        # optimiser and the published plans
        self._opt_calls_factory = b.optimizer_factory()
        self._plan_fwd_noise = b.forward_plan(True, True)         # forward(): complete outputs
        self._plan_fwd = b.forward_plan(False, True)
        self._plan_fwd_train = b.train_forward_plan()
        self._plan_bwd = b.bwd
        self._grad_buckets = b.grad_buckets()
        self._plan_opt = self._opt_calls_factory(1.0)
        self._plan_bwd_riders = self._plan_opt_rest = self._fold = self._fold_early = None
        ridden = b.riders()
        if ridden is not None:
            self._plan_bwd_riders, self._plan_opt_rest, r_lo = ridden
            self._fold_closing_update(self._plan_bwd_riders, r_lo, b.tail_mult)

    def _fold_closing_update(self, riders, r_lo, tail_mult):
        """The closing launch of the single-GPU latency-regime step (air_step_epilogue over the head [0, r_lo) of the flat
        buffers -- input encoder + LSTM, whose gradients the last launches of the backward form) disappears: the weight-gradient
        problems of the LAST backward launch apply centred RMSProp to the elements they finish, in the same epilogue
        (air_gemm_grouped_opt: on one GPU a tile's gradient is final when formed; nothing in that launch reads a parameter), and
        whatever else of the head was final before it rides as extra workgroups of the same launch, one of which advances the
        step counter and the Philox offset.  33 launches instead of 34 at BASELINE configs[1].  Applies when the head is made
        of whole float4 tensors that the last launch either forms or that earlier launches left final; otherwise the plan keeps
        its closing launch.  AIR_OPT_FOLD=0 switches it off (A/B).  The eligibility rules are gemm_groups'."""
        if _env("AIR_OPT_FOLD", "1") != "1" or self._use16:
            return
        L, dp = H.lib(), (lambda t: t.data_ptr())
        g0 = self.flat_grads.data_ptr()
        p0, p1 = self.flat_params.data_ptr(), self.flat_params.data_ptr() + 4 * self.n_total
        head = [(self.param_offsets[k], self.param_sizes[k]) for k in self.param_shapes if self.param_offsets[k] < r_lo]
        if any(sz % 4 for _, sz in head) or sum(sz for _, sz in head) != r_lo:
            return                                   # padding inside the head: the closing launch stays
        spans = sorted((self.param_offsets[k], self.param_offsets[k] + self.param_sizes[k]) for k in self.param_shapes)
        wide_min_tiles = int(_env("AIR_GEMM_WIDE_MIN_TILES", "1000"))
        shortk_on, shortk_min_m = _env("AIR_GEMM_SHORTK", "1") != "0", int(_env("AIR_GEMM_SHORTK_MIN_M", "4096"))

        def problems_to_fold(entry):
            """the problems of a grouped launch the library's folded form takes, else None"""
            if entry[2] != "air_gemm_grouped":
                return None
            descs = list(entry[1][0])
            if G.wide_form(descs, wide_min_tiles) or G.shortk_mixed(descs, shortk_on, shortk_min_m):
                return None
            return descs

        def disjoint(cov):
            cov = sorted(cov)
            return all(b0 >= a1 for (a0, a1), (b0, b1) in zip(cov, cov[1:]))

        last = riders[-1]
        last_p = problems_to_fold(last)
        # the closing launch folds what it forms; nothing in it may read a parameter at all (the rider workgroups behind its tiles
        # update the rest of the head, whatever it is)
        if last_p is None or G.tensors_read(last_p, p0, p1, spans):
            return
        mask_b, cov_b = G.foldable(last_p, g0, r_lo, [])
        if not mask_b:
            return
        # the launch in front of it (it holds the LSTM's weight gradients): folds the problems whose parameters neither
        # it nor the closing launch reads (its dX problem reads ITS layer's weights -- that layer's update stays with the closing launch)
        prev, mask_a, cov_a = None, 0, []
        prev_p = problems_to_fold(riders[-2]) if self._lstm_dw_early and len(riders) >= 2 else None
        if prev_p is not None:
            prev = riders[-2]
            mask_a, cov_a = G.foldable(prev_p, g0, r_lo, G.tensors_read(prev_p, p0, p1, spans))
            if not mask_a or not disjoint(cov_a + cov_b):
                prev, mask_a, cov_a = None, 0, []
        covered = sorted(cov_a + cov_b)
        if not disjoint(covered):
            return                                   # overlapping outputs: not a layout this fold understands
        ranges, cur = [], 0
        for a0, a1 in covered + [(r_lo, r_lo)]:
            if a0 > cur:
                ranges.append((cur, a0))
            cur = max(cur, a1)
        if len(ranges) > 4 or any(lo % 4 or hi % 4 for lo, hi in ranges):
            return
        cfg = self.cfg

        def make_fold(mask, rngs, counters):
            fold = _lib.AirOptFold()
            fold.p, fold.g, fold.ms, fold.mg, fold.mom = (dp(self.flat_params), g0, dp(self.flat_ms), dp(self.flat_mg), dp(self.flat_mom))
            fold.n_model = self.n_model
            fold.lr_dev = dp(self.lr_dev)
            fold.lr_mult_tail, fold.decay, fold.momentum, fold.eps, fold.grad_scale = (tail_mult, cfg.rms_decay, cfg.rms_momentum, cfg.rms_eps, 1.0)
            fold.fold_mask, fold.n_ranges = mask, len(rngs)
            for j, (lo, hi) in enumerate(rngs):
                fold.range_lo[j], fold.range_hi[j] = lo, hi
            if counters:
                fold.global_step_dev, fold.rng_state_dev, fold.rng_increment = dp(self.step_dev), dp(self.rng_state), self._rng_inc
            self._keep.append(fold)
            return fold

        riders = list(riders)
        if prev is not None:
            self._fold_early = make_fold(mask_a, [], False)          # (no rider slices, the counters move in the closing launch)
            riders[-2] = (L.air_gemm_grouped_opt, (prev[1][0], prev[1][1], ctypes.byref(self._fold_early)), "air_gemm_grouped_opt")
        self._fold = make_fold(mask_b, ranges, True)
        riders[-1] = (L.air_gemm_grouped_opt, (last[1][0], last[1][1], ctypes.byref(self._fold)), "air_gemm_grouped_opt")
        self._plan_bwd_riders = riders
        self._plan_opt_rest = []
