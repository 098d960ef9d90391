"""bf16 mirror bookkeeping of the throughput regime's bf16 data path (mixed into engine.AIREngine next to engine_plan.PlanMixin): the
mirrors and their address map, the pass that gives every grouped-GEMM descriptor of finished plans its mirrors, the parameter shadow,
and the dX-chain pass (AIR_DX_CHAIN=1, off by default).  Both passes rewrite finished launch lists by design: they apply to every
grouped launch whatever phase built it."""
import ctypes
import os

import torch

from . import _lib
from . import hip as H


class MirrorMixin:
    def _alloc_bf16_mirrors(self):
        """bf16 mirrors (same shape) of every buffer ALL of whose writers keep the mirror up to date -- see _apply_bf16_mirrors"""
        if getattr(self, "_mirror_spans", None) is not None:
            return
        dev, bf = self.device, torch.bfloat16
        self.flat_params16 = torch.zeros(self.n_total, dtype=bf, device=dev)
        self.obs16 = torch.zeros(self.obs.shape, dtype=bf, device=dev)
        self.h_seq16 = torch.zeros(self.h_seq.shape, dtype=bf, device=dev)
        self.dgates16 = torch.zeros(self.dgates.shape, dtype=bf, device=dev)
        self.dgx16 = torch.zeros(self.dgx.shape, dtype=bf, device=dev)
        self._mirror_of = {}
        trusted = [(self.flat_params, self.flat_params16), (self.obs, self.obs16)]
        # the LSTM's products: h_1..h_T (h_0 is the tiled initial state, written by the prologue: no mirror), dgates, running dgx
        lstm16 = self._lstm16_ok()
        if lstm16:
            trusted += [(self.h_seq[1:], self.h_seq16[1:]), (self.dgates, self.dgates16)]
            if self.T > 1:
                trusted.append((self.dgx, self.dgx16))
        gemm_made = []
        for m in (self.enc, self.ge, self.gd, self.bl):
            gemm_made += list(m.out)
        for m in (self.tr, self.st):     # the heads' output layers are written by air_attend_fwd when it is fused (and no product
            gemm_made += list(m.out[:-1])  # reads them as an operand either way): no mirror to trust
        for m in (self.enc, self.ge, self.gd, self.bl):      # (transform / steps: attend_bwd writes part of their gradient chain)
            gemm_made += list(m.g[:-1])
        gemm_made += [self.ge.g[-1], self.enc.g[-1]]
        for t in gemm_made:
            self._mirror_of[t.data_ptr()] = torch.zeros(t.shape, dtype=bf, device=dev)
            trusted.append((t, self._mirror_of[t.data_ptr()]))
        self._gemm_made = gemm_made
        self._mirror_spans = [(t.data_ptr(), t.data_ptr() + 4 * t.numel(), m16.data_ptr()) for t, m16 in trusted]

    def _lstm16_ok(self):
        """the shapes air_lstm_step_*_bf16 take (the library's wide-tile LSTM form)"""
        Hd, E = self.cfg.n_hidden, int(self.cfg.inpt_encoder_hidden[-1])
        # (the same threshold _build_plans uses for `fuse_lstm`: below it the fp32 fused steps run and write no mirror)
        return (((self.B + 15) // 16) * ((Hd + 15) // 16) > int(os.environ.get("AIR_FUSE_LSTM_TILES", "512"))
                and Hd % 64 == 0 and E % 4 == 0
                and os.environ.get("AIR_FUSE_LSTM_WIDE", "1") == "1" and os.environ.get("AIR_BF16_LSTM", "1") == "1")

    def _mirror_ptr(self, t):
        """address of the bf16 mirror of tensor / address `t` (None if it has none)"""
        ptr = t.data_ptr() if torch.is_tensor(t) else (int(t) if t else 0)
        if not ptr:
            return None
        for lo, hi, base16 in self._mirror_spans:
            if lo <= ptr < hi:
                return ctypes.c_void_p(base16 + (ptr - lo) // 2)
        return None

    def _apply_bf16_mirrors(self, plans):
        """bf16 data path: give every GEMM descriptor of `plans` the bf16 mirrors of its operands and of its output.

        Mirrored buffers (same shape, bf16): the flat parameter buffer (`flat_params16`: refreshed by every writer of the
        parameters -- the optimiser launch, load_parameters / init / load_state_dict), the observation batch (`obs16`: a convert
        launch at the start of every forward), the activations / gradients whose ONLY writers are GEMM epilogues -- each
        MLP's layer outputs and the hidden-layer gradients of the chains that GEMMs produce end to end (the library writes the
        mirror of C on every bf16 code path when the descriptor names one) -- and the LSTM's h_1..h_T, dgates and running dgx
        (air_lstm_step_*_bf16 write them).  Whatever another kernel writes (sampled latents, glimpses, the gradients the loss
        kernels hand to the chains, the tiled initial state) has no mirror: those operands are fetched as fp32 and rounded in
        registers, as before.  The values a product sees are identical either way (the mirror
        holds bf16(x), the register path computes bf16(x)); only the bytes moved change.  The caller refreshes the parameter shadow
        (_sync_param_shadow) and puts the conversion of obs in front of the forward."""
        out_spans = [(t.data_ptr(), t.data_ptr() + 4 * t.numel()) for t in self._gemm_made]

        def mirror(ptr):
            m = self._mirror_ptr(ptr)
            return m.value if m is not None else None

        for plan in plans:
            for e in plan:
                if e[2] != "air_gemm_grouped":
                    continue
                for d in e[1][0]:
                    d.A16, d.B16 = mirror(d.A), mirror(d.B)
                    c = int(d.C) if d.C else 0
                    d.C16 = mirror(c) if any(lo <= c < hi for lo, hi in out_spans) else None

    def _fuse_dx_chains(self, plan):
        """bf16 data path, throughput regime (round 6): runs of consecutive grouped-GEMM launches whose dX problems feed each other
        -- layer after layer of an MLP's backward, dA_{l-1} = (dA_l . W_l^T) * elu'(out_{l-1}) -- become ONE row-slab launch
        (air_mlp_dx_chain_bf16: a workgroup walks the whole chain for its 16 rows; nothing crosses rows).  A chain starts at a dX
        problem whose input no earlier problem of the run produces and is placed where its first layer was (every later layer only
        needs the layer before it and saved activations, so running it earlier is safe); problems that are not part of a chain of at
        least two layers stay in their grouped launch.  Same values as the per-layer launches up to the order of the fp32
        accumulation (each layer reads bf16 of the previous fp32 result either way)."""
        L = H.lib()
        MDELU, NONE = H.EPI_MUL_DELU, H.EPI_NONE

        def dx_ok(d):
            return (not d.ta and d.tb and d.epilogue in (MDELU, NONE) and d.beta == 0.0 and not d.A2 and not d.colsum and not d.bias
                    and d.B16 and d.ldb == d.K and (d.epilogue == NONE or d.aux) and L.air_mlp_dx_chain_fits(d.K, d.N) == 1)

        out, i = [], 0
        while i < len(plan):
            e = plan[i]
            if e[2] != "air_gemm_grouped":
                out.append(e); i += 1
                continue
            j = i
            while j < len(plan) and plan[j][2] == "air_gemm_grouped":
                j += 1
            launches = [[x[1][0][q] for q in range(x[1][1])] for x in plan[i:j]]
            chains = []                                      # [first launch index, last launch index, [descs]]
            for a_idx, ds in enumerate(launches):
                for d in ds:
                    if not dx_ok(d):
                        continue
                    host = None
                    for c in chains:
                        t = c[2][-1]
                        if (c[1] < a_idx and len(c[2]) < 4 and int(d.A) == int(t.C) and d.lda == t.ldc and d.K == t.N and d.M == t.M):
                            host = c
                            break
                    if host is not None:
                        host[2].append(d); host[1] = a_idx
                    else:
                        chains.append([a_idx, a_idx, [d]])
            chains = [c for c in chains if len(c[2]) >= 2]
            fused = {id(d) for c in chains for d in c[2]}
            for a_idx, ds in enumerate(launches):
                starts = [c for c in chains if c[0] == a_idx]
                for k0 in range(0, len(starts), 4):
                    grp = starts[k0:k0 + 4]
                    arr = (_lib.AirDxChain * len(grp))()
                    for ci, c in enumerate(grp):
                        d0 = c[2][0]
                        arr[ci].g_in, arr[ci].ld_in, arr[ci].rows, arr[ci].n_layers = d0.A, d0.lda, d0.M, len(c[2])
                        for li, d in enumerate(c[2]):
                            y = arr[ci].layer[li]
                            y.w_bf16, y.aux, y.out, y.out_bf16 = d.B16, (d.aux if d.epilogue == MDELU else None), d.C, d.C16
                            y.n_in, y.n_out, y.ldaux, y.ldout = d.K, d.N, d.ldaux, d.ldc
                    self._keep.append(arr)
                    out.append((L.air_mlp_dx_chain_bf16, (arr, len(grp)), "air_mlp_dx_chain_bf16"))
                    self._dx_chain_launches += 1
                rest = [d for d in ds if id(d) not in fused]
                if rest:
                    arr = (_lib.AirGemmDesc * len(rest))(*rest)
                    self._keep.append(arr)
                    out.append((L.air_gemm_grouped, (arr, len(rest)), "air_gemm_grouped"))
            i = j
        return out

    def _sync_param_shadow(self):
        """bf16 shadow of the parameters after anything but the optimiser launch wrote them"""
        if getattr(self, "flat_params16", None) is not None:
            st = H.lib().air_f32_to_bf16(H._p(self.flat_params), ctypes.c_void_p(self.flat_params16.data_ptr()),
                                         ctypes.c_size_t(self.n_total), self._sp())
            _lib.check(st, "air_f32_to_bf16")
