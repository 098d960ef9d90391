// fp32 MFMA GEMM for the small, weight-resident layers of AIR (snt.Linear / snt.LSTM matmuls: neural.py:42-60,
// mnist_model.py:35; backward of the same).  C[M,N] = epi(op(A)[M,K].op(B)[K,N] + beta*C).
//
// Regime: M = B or T*B rows (64..3072), K,N in {1..3177}; all weights (10.5 MB) live in L2 / Infinity Cache, so at
// the headline batch the problem is latency/occupancy bound, not HBM bound.  Design for that:
//   * v_mfma_f32_16x16x4_f32 (exact fp32 fma chain; 157 TF peak = the fp32 vector rate, no TF32 on gfx950).
//   * operands go global -> VGPR directly in MFMA fragment order, no LDS staging: lane (i = l&15, g = l>>4)
//     supplies k = kc + 4g + j in MFMA step j for BOTH A and B, so a k-contiguous operand is one 16-byte load per
//     lane per 16-deep chunk and a k-strided operand is four dword loads covering 64-byte row segments.
//   * occupancy from split-K: the 4 waves of a workgroup interleave 16-deep K chunks of one output tile and reduce
//     through LDS (deterministic); a second, cross-workgroup split writes fp32 slabs that a small epilogue kernel
//     sums in a fixed order (no atomics => bitwise reproducible run to run).
//   * epilogues fuse bias, ELU, ELU' (backward), residual add; the dW form fuses the bias gradient (column sums).
// Arbitrary M/N/K and leading dimensions are handled with masked edge loads (test/cell_test.py uses 3x3 images and
// hidden sizes 5/7/11/13/17).
#include "air_common.h"
#include "prologue_device.h"
#include "optimizer_device.h"
#include "engine_device.h"
#include "nvil_device.h"
#include "gemm_device.h"
#include <cstring>
#include <type_traits>


// consumer-side reduction of a K-split producer (AirGemmDesc.A2 ...): a separate kernel argument of the one kernel that uses it --
// every field added to GemmArgs is loaded by EVERY GEMM launch (x8 in a grouped launch): five more cost 7 us per step, measured
struct AproArgs {
    const float *A2, *a_bias;
    float *a_out;
    int a_elu;
};
// the centred-RMSProp update folded into the epilogue of the weight-gradient tiles that FORM the gradients (single GPU: a tile's
// gradient is final when formed), plus rider workgroups for slices whose gradients earlier launches left final, plus the step
// counters: the closing launch of the train step disappears (air_gemm_grouped_opt).  A separate kernel argument of the kernels
// that use it, like AproArgs.
#define AIR_OPT_MAX_RANGES 4
struct OptFold {
    float *p; const float *g0; float *ms, *mg, *mom;       // bases of the flat buffers; g0: the flat gradient buffer C / colsum point into
    size_t n_model;
    const float *lr_dev;
    float lr_mult_tail, decay, momentum, eps, gscale;
    unsigned fold_mask;                                     // bit i: problem i's C and colsum elements are updated where they are formed
    int n_ranges, tiles;                                    // rider slices [lo, hi) (multiples of 4); workgroups >= tiles are riders
    size_t lo[AIR_OPT_MAX_RANGES], hi[AIR_OPT_MAX_RANGES];
    int64_t *gstep; uint64_t *rng_state; uint64_t rng_inc;
};
// the rider workgroups of such a launch (blockIdx.x >= OPT_.tiles): each takes its share of every rider slice, the first one advances
// the counters.  A macro, not a function: as a __device__ __forceinline__ function taking the OptFold by reference it left the
// resource usage of gemm_grouped_opt_kernel / gemm_grouped_opt_sk_kernel alone but not their instructions (the rider's scalar
// prologue came out differently in all seven); the macro expands to the tokens that stood in each kernel, and they compile as before.
#define AIR_OPT_RIDERS(OPT_)                                                                                                     \
    if ((int)blockIdx.x >= OPT_.tiles) {                                                                                         \
        const int vb = (int)blockIdx.x - OPT_.tiles, vg = (int)gridDim.x - OPT_.tiles;                                           \
        for (int r = 0; r < OPT_.n_ranges; ++r) {                                                                                \
            RmspropSlice sl;                                                                                                     \
            sl.p = OPT_.p; sl.g = OPT_.g0; sl.ms = OPT_.ms; sl.mg = OPT_.mg; sl.mom = OPT_.mom;                                  \
            sl.lo = OPT_.lo[r]; sl.hi = OPT_.hi[r]; sl.n_model = OPT_.n_model; sl.lr_dev = OPT_.lr_dev;                          \
            sl.lr_mult_tail = OPT_.lr_mult_tail; sl.decay = OPT_.decay; sl.momentum = OPT_.momentum; sl.eps = OPT_.eps;          \
            sl.gscale = OPT_.gscale;                                                                                             \
            rmsprop_slice_body(sl, vb, vg);                                                                                      \
        }                                                                                                                        \
        if (vb == 0 && threadIdx.x == 0) {                                                                                       \
            if (OPT_.gstep) OPT_.gstep[0] += 1;                                                                                  \
            if (OPT_.rng_state) OPT_.rng_state[1] += OPT_.rng_inc;                                                               \
        }                                                                                                                        \
        return;                                                                                                                  \
    }
// the backward of a Gaussian head (loc_mode 0: the `what` head) folded into the epilogue of the product that forms its sample
// gradient (the decoder's first-layer dX, d_what[T*B, D]): the tile's element (m, d) IS dsample[m, d], and the thread that finished it
// writes dpre[m, d] and dpre[m, D + d] (engine_device.h gauss_bwd_elem) instead of storing it for a pointwise launch to re-read.
struct GaussEpi {
    const float *pre, *eps, *loc, *scale, *dkl_row;
    float *dpre;
    int ld_pre, ld_dpre, D;
    float raw_offset, pl, ps, dkl_scale, guard;
    unsigned mask;                                          // bit i: problem i carries the epilogue
};
// The HBM feeder's gather folded into the step's FIRST product (round 6): the problems of that launch contract over the pixels of the
// observation batch, so row m of their A operand is read straight from item idx_m of the resident dataset -- idx_m drawn exactly as
// air_batch_gather draws it (Philox(seed, stream 1, counter step*B + m), or the sequential walk) -- and the first column of tiles of the
// problems in copy_mask writes the fragments it loaded into the observation buffer, which every later launch of the step reads as before.
// One dependent launch less at the head of the step.  A separate kernel argument of the one kernel that uses it, like AproArgs.
struct GatherArgs {
    const float *data, *obs;
    float *obs_out;
    long long n_items;
    int item_floats, shuffle, B;
    const uint64_t *seed;
    const int64_t *step;
    int64_t *idx_out;
    unsigned copy_mask;
};
__device__ __forceinline__ long long gather_item(const GatherArgs &gt, int m) {
    const unsigned long long ctr = (unsigned long long)gt.step[0] * (unsigned long long)gt.B + (unsigned long long)m;
    if (gt.shuffle) {
        uint32_t r[4];
        philox4x32(ctr, 1, gt.seed[0], r);
        const unsigned long long wide = ((unsigned long long)r[0] << 32) | r[1];
        return (long long)(((unsigned __int128)wide * (unsigned __int128)gt.n_items) >> 64);        // uniform in [0, n)
    }
    return (long long)(ctr % (unsigned long long)gt.n_items);
}
struct GemmArgs {
    const float *A, *B, *bias, *aux;
    float *C, *colsum, *ws;
    int M, N, K, lda, ldb, ldc, ldaux;
    int ta, tb, epi, S, chunks_per_split, vecA, vecB;
    float beta;
};


__device__ __forceinline__ float apply_epilogue(float v, int m, int n, const GemmArgs &g) {
    if (g.beta != 0.f) v += g.beta * g.C[(size_t)m * g.ldc + n];
    switch (g.epi) {
        case AIR_EPI_BIAS: v += g.bias[n]; break;
        case AIR_EPI_BIAS_ELU: v = elu_acc(v + g.bias[n]); break;
        case AIR_EPI_MUL_DELU: {
            const float y = g.aux[(size_t)m * g.ldaux + n];
            v *= (y > 0.f ? 1.f : y + 1.f);
        } break;
        case AIR_EPI_ADD_AUX:
            v += g.aux[(size_t)m * g.ldaux + n];
            if (g.bias) v += g.bias[n];
            break;
        case AIR_EPI_ADD_AUX_ELU:
            v += g.aux[(size_t)m * g.ldaux + n];
            if (g.bias) v += g.bias[n];
            v = elu_acc(v);
            break;
        default: break;
    }
    return v;
}

// MT x NT 16x16 MFMA tiles per wave.  KW = 4 / 16: the workgroup's KW waves split K for ONE tile (LDS reduce; 16
// waves = 1024 threads for long-K problems with few tiles, so no second split-K launch is needed);
// KW = 1: the 4 waves own 4 neighbouring N-tiles.
// HALF (<1, 1, 16> only, gemm_grouped_longk_half_kernel): the workgroup OWNS own_r x own_c (8x16 / 8x8 / 16x16, wave-uniform, per problem)
// of its MFMA tile.  Lanes li >= own_r (own_c) issue NO operand load in the full chunks (zero fragments) and the accumulator rows /
// columns they feed are never read.  An owned element keeps its K chunks, the order inside a chunk and the reduction over the waves:
// the bits of the 16x16 tile.
template <int MT, int NT, int KW, bool BF, bool APRO = false, bool OPT = false, bool GBW = false, bool GATH = false, bool HALF = false>
__device__ __forceinline__ void gemm_body(const GemmArgs &g, const int block_tile, const int split, const AproArgs pro = AproArgs(),
                                          void *c16 = nullptr, const OptFold *opt = nullptr, const bool fold = false,
                                          const GaussEpi *gb = nullptr, const GatherArgs *gt = nullptr, const bool gcopy = false,
                                          const int own_r = 16, const int own_c = 16) {
    static_assert(!HALF || (MT == 1 && NT == 1 && KW == 16 && !APRO && !OPT && !GBW && !GATH), "half tiles: the plain 16-wave body only");
    const gh_t hC = (gh_t)c16;             // bf16 mirror of C (bf16 data path: the next product reads it instead of the fp32 value)
    constexpr int TM = 16 * MT, TN = 16 * NT;
    constexpr int NWN = (KW == 1) ? 4 : 1;               // waves across N
    constexpr int NWV = (KW == 1) ? 4 : KW;               // waves per workgroup
    constexpr int NTH = 64 * NWV;                         // threads per workgroup
    constexpr int LDT = TN + 4;                           // padded LDS tile row
    __shared__ float s_tile[NWV][TM * LDT];
    __shared__ float s_col[NWV][TN];

    const gcf gA = (gcf)g.A, gB = (gcf)g.B, gBias = (gcf)g.bias, gAux = (gcf)g.aux;
    const gf gC = (gf)g.C, gWs = (gf)g.ws, gCol = (gf)g.colsum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int OWN_M = HALF ? own_r : TM, OWN_N = HALF ? own_c : TN;        // (not HALF: the constants they were)
    const int tiles_n = (g.N + OWN_N * NWN - 1) / (OWN_N * NWN);
    const int tm = block_tile / tiles_n, tn = block_tile - tm * tiles_n;
    const int m0 = tm * OWN_M;
    const int n0 = (tn * NWN + (KW == 1 ? wave : 0)) * OWN_N;
    const int own_sh = own_c == 8 ? 3 : 4;                                // e / own_c

    const int total_chunks = (g.K + 15) >> 4;
    const int c_begin = split * g.chunks_per_split;
    int c_end = c_begin + g.chunks_per_split;
    if (c_end > total_chunks) c_end = total_chunks;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float csum[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) csum[b] = 0.f;
    const bool want_colsum = (g.colsum != nullptr) && (tm == 0);

    int rowA[MT], colB[NT];
    bool okA[MT], okB[NT];
#pragma unroll
    for (int a = 0; a < MT; ++a) { rowA[a] = m0 + 16 * a + li; okA[a] = rowA[a] < g.M && (!HALF || li < own_r); }
#pragma unroll
    for (int b = 0; b < NT; ++b) { colB[b] = n0 + 16 * b + li; okB[b] = colB[b] < g.N && (!HALF || li < own_c); }

    // Epilogue operands (bias / aux / beta*C) are fetched NOW, before the K loop, so their memory round trip overlaps
    // the operand loads instead of following the LDS reduction (the kernel is a chain of round trips, not of flops).
    constexpr int EPT = (KW > 1) ? (TM * TN + NTH - 1) / NTH : 1;
    float e_bias[EPT], e_aux[EPT], e_c[EPT];
    if (KW > 1 && g.S == 1) {
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = threadIdx.x + NTH * i;
            const int r = HALF ? (e >> own_sh) : e / TN, cidx = e - r * OWN_N;
            const int m = m0 + r, n = n0 + cidx;
            const bool ok = (e < OWN_M * OWN_N) && m < g.M && n < g.N;
            e_bias[i] = (ok && g.bias != nullptr) ? gBias[n] : 0.f;
            e_aux[i] = (ok && g.epi >= AIR_EPI_MUL_DELU) ? gAux[(size_t)m * g.ldaux + n] : 0.f;
            e_c[i] = (ok && g.beta != 0.f) ? gC[(size_t)m * g.ldc + n] : 0.f;
        }
    }
    // Gaussian-head backward in the epilogue: its operands are requested NOW as well
    float b_loc[GBW ? EPT : 1], b_scale[GBW ? EPT : 1], b_eps[GBW ? EPT : 1], b_raw[GBW ? EPT : 1], b_dk[GBW ? EPT : 1];
    if (GBW && KW > 1 && fold) {
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = threadIdx.x + NTH * i;
            const int r = HALF ? (e >> own_sh) : e / TN, cidx = e - r * OWN_N;
            const int m = m0 + r, n = n0 + cidx;
            const bool ok = (e < OWN_M * OWN_N) && m < g.M && n < g.N;
            const size_t o = ok ? (size_t)m * gb->D + n : 0;
            b_loc[i] = ok ? ((gcf)gb->loc)[o] : 0.f;
            b_scale[i] = ok ? ((gcf)gb->scale)[o] : 1.f;
            b_eps[i] = ok ? ((gcf)gb->eps)[o] : 0.f;
            b_raw[i] = ok ? ((gcf)gb->pre)[(size_t)m * gb->ld_pre + gb->D + n] : 0.f;
            b_dk[i] = (ok && gb->dkl_row) ? ((gcf)gb->dkl_row)[m] : 0.f;
        }
    }
    // folded update: the element's parameter and RMSProp slots are requested NOW, with the operands (same flat offset as its gradient)
    float o_p[OPT ? EPT : 1], o_ms[OPT ? EPT : 1], o_mg[OPT ? EPT : 1], o_mom[OPT ? EPT : 1];
    float o_lr0 = 0.f;
    if (OPT && KW > 1 && fold) {
        o_lr0 = ((gcf)opt->lr_dev)[0];
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = threadIdx.x + NTH * i;
            const int r = HALF ? (e >> own_sh) : e / TN, cidx = e - r * OWN_N;
            const int m = m0 + r, n = n0 + cidx;
            const bool ok = (e < OWN_M * OWN_N) && m < g.M && n < g.N;
            const size_t idx = ok ? (size_t)((gC + (size_t)m * g.ldc + n) - (gf)opt->g0) : 0;
            o_p[i] = ok ? ((gf)opt->p)[idx] : 0.f;
            o_ms[i] = ok ? ((gf)opt->ms)[idx] : 0.f;
            o_mg[i] = ok ? ((gf)opt->mg)[idx] : 0.f;
            o_mom[i] = ok ? ((gf)opt->mom)[idx] : 0.f;
        }
    }

    const int c_step = (KW > 1) ? KW : 1;
    int c = c_begin + ((KW > 1) ? wave : 0);
    // ---- main loop: U chunks in flight per wave.  The problem is latency bound (operands sit in L2 / Infinity
    // Cache, each wave owns only a handful of 16-deep chunks), so all loads of U chunks are issued before the first
    // MFMA: one memory round trip per U chunks instead of one per chunk.
    constexpr int U = (MT * NT == 1) ? (KW == 16 ? 10 : 8) : 4;   // chunks in flight: small tiles can afford more registers
    int full_end = g.K >> 4;                               // chunks [0, full_end) need no k masking
    if (full_end > c_end) full_end = c_end;
    int rowAc[MT], colBc[NT];
#pragma unroll
    for (int a = 0; a < MT; ++a) rowAc[a] = okA[a] ? rowA[a] : g.M - 1;
#pragma unroll
    for (int b = 0; b < NT; ++b) colBc[b] = okB[b] ? colB[b] : g.N - 1;
    // GATH: row m of A = item idx_m of the dataset, at the problem's column offset inside an observation row (A points into row 0 of obs)
    const int gcol = GATH ? (int)(gA - (gcf)gt->obs) : 0;
    const gcf gAs = GATH ? (gcf)gt->data + gcol : gA;
    const int ldAs = GATH ? gt->item_floats : g.lda;
    int rowAs[MT];
#pragma unroll
    for (int a = 0; a < MT; ++a) rowAs[a] = GATH ? (int)gather_item(*gt, rowAc[a]) : rowAc[a];
    if (GATH && gcopy && tn == 0 && split == 0 && wave == 0 && lg == 0 && gt->idx_out && gcol == 0) {
#pragma unroll
        for (int a = 0; a < MT; ++a) if (okA[a]) gt->idx_out[rowA[a]] = rowAs[a];
    }
#pragma nounroll
    for (; c < full_end; c += U * c_step) {   // (unrolling this loop doubles the live operand registers: 94 -> 194 VGPRs)
        f32x4 fa[U][MT], fb[U][NT];
        f32x4 fa2[APRO ? U : 1][APRO ? MT : 1], fab[APRO ? U : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cu = c + u * c_step;
            if (cu < full_end) {                           // wave-uniform: a short tail group issues fewer loads
                const int k = (cu << 4) + 4 * lg;
#pragma unroll
                for (int a = 0; a < MT; ++a) {
                    if (HALF && !okA[a]) { fa[u][a] = (f32x4){0.f, 0.f, 0.f, 0.f}; continue; }     // (outside the owned rows: no load)
                    fa[u][a] = g.ta ? ld_kstrided_full(gA, g.lda, rowAc[a], k)
                                    : ld_kcontig_full(gAs, ldAs, rowAs[a], k, g.vecA != 0);
                    if (APRO) {       // second K-split slab + bias of the producing layer: requested with the operand itself
                        fa2[u][a] = ld_kcontig_full((gcf)pro.A2, g.lda, rowAc[a], k, g.vecA != 0);
                        fab[u] = ld_kcontig_full((gcf)pro.a_bias, 0, 0, k, g.vecA != 0);
                    }
                }
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    if (HALF && !okB[b]) { fb[u][b] = (f32x4){0.f, 0.f, 0.f, 0.f}; continue; }
                    fb[u][b] = g.tb ? ld_kcontig_full(gB, g.ldb, colBc[b], k, g.vecB != 0)
                                    : ld_kstrided_full(gB, g.ldb, colBc[b], k);
                }
            } else {
#pragma unroll
                for (int a = 0; a < MT; ++a) fa[u][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < NT; ++b) fb[u][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * c_step >= full_end) break;
            if (APRO) {
#pragma unroll
                for (int a = 0; a < MT; ++a) {
                    f32x4 v = (fa[u][a] + fa2[u][a]) + fab[u];
                    if (pro.a_elu) { v.x = elu_acc(v.x); v.y = elu_acc(v.y); v.z = elu_acc(v.z); v.w = elu_acc(v.w); }
                    fa[u][a] = v;
                    if (pro.a_out != nullptr && tn == 0 && okA[a])        // the reduced activation, for the backward pass
                        *(f32x4 *)(pro.a_out + (size_t)rowA[a] * g.lda + (((c + u * c_step) << 4) + 4 * lg)) = v;
                }
            }
            if (GATH && gcopy && tn == 0) {                // the gathered rows, for every later reader of the observation batch
#pragma unroll
                for (int a = 0; a < MT; ++a)
                    if (okA[a]) *(f32x4 *)(gt->obs_out + (size_t)rowA[a] * g.lda + gcol + (((c + u * c_step) << 4) + 4 * lg)) = fa[u][a];
            }
            mfma_chunk<MT, NT, BF>(acc, fa[u], fb[u]);
            if (want_colsum) {
#pragma unroll
                for (int b = 0; b < NT; ++b)
                    csum[b] += okB[b] ? (fb[u][b].x + fb[u][b].y) + (fb[u][b].z + fb[u][b].w) : 0.f;
            }
        }
    }
    // ---- the partial last chunk of K (if any), fully masked, done by the wave that owns it
    const int pc = g.K >> 4;
    if ((g.K & 15) && pc >= c_begin && pc < c_end && (KW == 1 || ((pc - c_begin) % KW) == wave)) {
        const int k = (pc << 4) + 4 * lg;
        f32x4 fa[MT], fb[NT];
#pragma unroll
        for (int a = 0; a < MT; ++a)
            fa[a] = g.ta ? ld_kstrided(gA, g.lda, rowA[a], okA[a], k, g.K)
                         : ld_kcontig(gAs, ldAs, GATH ? rowAs[a] : rowA[a], okA[a], k, g.K, g.vecA != 0);
        if (GATH && gcopy && tn == 0) {
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                if (!okA[a]) continue;
                float *d = gt->obs_out + (size_t)rowA[a] * g.lda + gcol + k;
                if (k < g.K) d[0] = fa[a].x;
                if (k + 1 < g.K) d[1] = fa[a].y;
                if (k + 2 < g.K) d[2] = fa[a].z;
                if (k + 3 < g.K) d[3] = fa[a].w;
            }
        }
#pragma unroll
        for (int b = 0; b < NT; ++b)
            fb[b] = g.tb ? ld_kcontig(gB, g.ldb, colB[b], okB[b], k, g.K, g.vecB != 0)
                         : ld_kstrided(gB, g.ldb, colB[b], okB[b], k, g.K);
        mfma_chunk<MT, NT, BF>(acc, fa, fb);
        if (want_colsum) {
#pragma unroll
            for (int b = 0; b < NT; ++b) csum[b] += (fb[b].x + fb[b].y) + (fb[b].z + fb[b].w);
        }
    }

    // accumulators -> LDS tile (C/D map: col = lane&15, row = (lane>>4)*4 + r)
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_tile[wave][(16 * a + 4 * lg + r) * LDT + 16 * b + li] = acc[a][b][r];
    if (want_colsum) {
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            float v = csum[b];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lg == 0) s_col[wave][16 * b + li] = v;
        }
    }
    __syncthreads();

    if (KW > 1) {
        // all threads reduce the KW per-wave partial tiles (fixed order) and finish one TM x TN tile
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = threadIdx.x + NTH * i;
            if (e >= OWN_M * OWN_N) continue;
            const int r = HALF ? (e >> own_sh) : e / TN, cidx = e - r * OWN_N;
            const int m = m0 + r, n = n0 + cidx;
            if (m >= g.M || n >= g.N) continue;
            const int off = r * LDT + cidx;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < NWV; q += 4)
                v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
            if (g.S > 1) {
                gWs[((size_t)split * g.M + m) * g.N + n] = v;
            } else {
                if (g.beta != 0.f) v += g.beta * e_c[i];
                switch (g.epi) {
                    case AIR_EPI_BIAS: v += e_bias[i]; break;
                    case AIR_EPI_BIAS_ELU: v = elu_acc(v + e_bias[i]); break;
                    case AIR_EPI_MUL_DELU: v *= (e_aux[i] > 0.f ? 1.f : e_aux[i] + 1.f); break;
                    case AIR_EPI_ADD_AUX: v += e_aux[i] + e_bias[i]; break;
                    case AIR_EPI_ADD_AUX_ELU: v = elu_acc(v + e_aux[i] + e_bias[i]); break;
                    default: break;
                }
                gC[(size_t)m * g.ldc + n] = v;
                if (BF && hC) hC[(size_t)m * g.ldc + n] = bf16_bits(v);
                if (GBW && fold) {                          // v = dsample[m, n] of the head: its pre-activation gradients, here
                    float dloc, draw;
                    gauss_bwd_elem(v, true, b_eps[i], b_loc[i], b_scale[i], gb->pl, gb->ps, b_dk[i] * gb->dkl_scale,
                                   b_raw[i] + gb->raw_offset, 0, n, gb->guard, dloc, draw);
                    const gf dp_ = (gf)gb->dpre + (size_t)m * gb->ld_dpre;
                    dp_[n] = dloc; dp_[gb->D + n] = draw;
                }
                if (OPT && fold) {
                    const size_t idx = (size_t)((gC + (size_t)m * g.ldc + n) - (gf)opt->g0);
                    const float lr = idx < opt->n_model ? o_lr0 : o_lr0 * opt->lr_mult_tail;
                    float pv = o_p[i], a = o_ms[i], b = o_mg[i], c = o_mom[i];
                    rmsprop_elem(pv, v, a, b, c, lr, opt->decay, opt->momentum, opt->eps, opt->gscale);
                    ((gf)opt->ms)[idx] = a; ((gf)opt->mg)[idx] = b; ((gf)opt->mom)[idx] = c; ((gf)opt->p)[idx] = pv;
                }
            }
        }
        if (want_colsum && threadIdx.x < TN) {
            const int n = n0 + threadIdx.x;
            if (n < g.N) {
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < NWV; q += 4)
                    v += (s_col[q][threadIdx.x] + s_col[q + 1][threadIdx.x]) + (s_col[q + 2][threadIdx.x] + s_col[q + 3][threadIdx.x]);
                gCol[n] = v;
                if (OPT && fold) {                          // the bias gradient this tile column finishes: same treatment
                    const size_t idx = (size_t)((gCol + n) - (gf)opt->g0);
                    const float lr = idx < opt->n_model ? o_lr0 : o_lr0 * opt->lr_mult_tail;
                    float pv = ((gf)opt->p)[idx], a = ((gf)opt->ms)[idx], b = ((gf)opt->mg)[idx], c = ((gf)opt->mom)[idx];
                    rmsprop_elem(pv, v, a, b, c, lr, opt->decay, opt->momentum, opt->eps, opt->gscale);
                    ((gf)opt->ms)[idx] = a; ((gf)opt->mg)[idx] = b; ((gf)opt->mom)[idx] = c; ((gf)opt->p)[idx] = pv;
                }
            }
        }
    } else {
        // each wave finishes its own tile
        for (int e = lane; e < TM * TN; e += 64) {
            const int r = e / TN, cidx = e - r * TN;
            const int m = m0 + r, n = n0 + cidx;
            if (m >= g.M || n >= g.N) continue;
            const float v = s_tile[wave][r * LDT + cidx];
            if (g.S > 1) gWs[((size_t)split * g.M + m) * g.N + n] = v;
            else {
                const float o = apply_epilogue(v, m, n, g);
                gC[(size_t)m * g.ldc + n] = o;
                if (BF && hC) hC[(size_t)m * g.ldc + n] = bf16_bits(o);
            }
        }
        if (want_colsum && lane < TN) {
            const int n = n0 + lane;
            if (n < g.N) gCol[n] = s_col[wave][lane];
        }
    }
}

template <int MT, int NT, int KW, bool BF>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_f32_mfma_kernel(GemmArgs g) {
    gemm_body<MT, NT, KW, BF>(g, blockIdx.x, blockIdx.y);
}
// bf16 data path, small tiles: fp32 operand fetch (rounded in registers) + the bf16 mirror of C
template <int MT, int NT, int KW>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_bf16_c16_kernel(GemmArgs g, void *c16) {
    gemm_body<MT, NT, KW, true>(g, blockIdx.x, blockIdx.y, AproArgs(), c16);
}
// the same body with the A-operand prologue (consumer-side reduction of a K-split producer) compiled in
template <int MT, int NT, int KW, bool BF>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_f32_mfma_apro_kernel(GemmArgs g, AproArgs pro) {
    gemm_body<MT, NT, KW, BF, true>(g, blockIdx.x, blockIdx.y, pro);
}

// ---- throughput regime (thousands of rows): "wide" wave tiles with every operand load 16 bytes per lane ---------------------
// gemm_body feeds a k-strided operand (forward: W[K,N]; weight gradient: both operands) with dword loads -- 64-byte segments, 16
// address cycles per wave instruction for 256 bytes: at batch 1024 the load path, not the MFMA pipe, bounds those products (the
// texture-address unit is busier than the matrix cores: 640 against 512 cycles per 16-deep chunk of a 32x32 tile, 4 waves per CU).
// Here a k-strided operand is read with ONE 16-byte load per lane ALONG ITS CONTIGUOUS DIMENSION, and the four values a lane gets
// are handed to FOUR DIFFERENT 16-wide MFMA tiles: tile t of a 64-wide block owns the INTERLEAVED columns n0 + 4 i + t (i = 0..15)
// instead of the contiguous columns n0 + 16 t + i.  MFMA does not care which column a lane's value belongs to, only that A and B
// agree on k; the accumulator of lane (i, g) then holds C[row][n0 + 4 i + 0..3] across the four tiles: a 16-byte store.  A
// k-contiguous operand keeps the block layout (one 16-byte load per lane per chunk along k).  Wave tile (16 MT) x 64: MT + 4
// 16-byte loads per 16-deep chunk feed 4 MT (bf16) or 16 MT (fp32) MFMAs; KW waves split K and reduce through LDS in fixed order.
template <int MT, int KW, bool BF, bool TA, bool TB>
__device__ __forceinline__ void gemm_wide_body(const GemmArgs &g, const int block_tile) {
    constexpr int NT = 4, TM = 16 * MT, TN = 64;
    constexpr int NTH = 64 * KW;
    constexpr int LDT = TN + 4;
    static_assert(!TA || MT == 4, "an m-contiguous A operand is read 4 rows per lane: four interleaved row tiles");
    __shared__ float s_tile[KW][TM * LDT];
    __shared__ float s_col[KW][TN];

    const gcf gA = (gcf)g.A, gB = (gcf)g.B, gBias = (gcf)g.bias, gAux = (gcf)g.aux;
    const gf gC = (gf)g.C, gCol = (gf)g.colsum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int tiles_n = (g.N + TN - 1) / TN;
    const int tm = block_tile / tiles_n, tn = block_tile - tm * tiles_n;
    const int m0 = tm * TM, n0 = tn * TN;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float csum[NT] = {0.f, 0.f, 0.f, 0.f};
    const bool want_colsum = TA && (g.colsum != nullptr) && (tm == 0);

    // operand addressing.  Block layout: tile t row/col 16 t + li, one address per tile.  Interleaved: rows/cols 4 li + t, ONE
    // address for all four tiles (clamped inside the matrix: lanes past the edge feed accumulators that are never stored; the
    // dispatcher guarantees M % 4 == 0 / N % 4 == 0 for an interleaved operand, so a lane is entirely inside or entirely outside)
    int offA[TA ? 1 : MT], offB[TB ? NT : 1];
    if (TA) { int r = m0 + 4 * li; if (r > g.M - 4) r = g.M - 4; offA[0] = r; }
    else {
#pragma unroll
        for (int a = 0; a < MT; ++a) { int r = m0 + 16 * a + li; if (r > g.M - 1) r = g.M - 1; offA[a] = r * g.lda; }
    }
    if (!TB) { int c = n0 + 4 * li; if (c > g.N - 4) c = g.N - 4; offB[0] = c; }
    else {
#pragma unroll
        for (int b = 0; b < NT; ++b) { int c = n0 + 16 * b + li; if (c > g.N - 1) c = g.N - 1; offB[b] = c * g.ldb; }
    }

    // epilogue operands requested before the K loop (their round trip hides under the operand loads)
    constexpr int EPT = (TM * TN) / NTH;
    static_assert((TM * TN) % NTH == 0, "tile / threads");
    float e_bias[EPT], e_aux[EPT], e_c[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = threadIdx.x + NTH * i;
        const int r = e / TN, cidx = e - r * TN;
        int m = m0 + r, n = n0 + cidx;
        if (m > g.M - 1) m = g.M - 1;
        if (n > g.N - 1) n = g.N - 1;
        e_bias[i] = g.bias != nullptr ? gBias[n] : 0.f;
        e_aux[i] = g.epi >= AIR_EPI_MUL_DELU ? gAux[(size_t)m * g.ldaux + n] : 0.f;
        e_c[i] = g.beta != 0.f ? gC[(size_t)m * g.ldc + n] : 0.f;
    }

    constexpr int U = (MT == 4) ? 3 : 4;                   // chunks in flight per wave
    const int full_end = g.K >> 4;
    auto load_chunk = [&](int k, f32x4 (&fa)[MT], f32x4 (&fb)[NT]) {       // k = first of the lane group's four k values
        if (TA) {
            f32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = *(gcf4)(gA + (size_t)(k + j) * g.lda + offA[0]);
#pragma unroll
            for (int a = 0; a < MT; ++a) fa[a] = (f32x4){v[0][a], v[1][a], v[2][a], v[3][a]};
        } else {
#pragma unroll
            for (int a = 0; a < MT; ++a) fa[a] = *(gcf4)(gA + offA[a] + k);
        }
        if (!TB) {
            f32x4 w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = *(gcf4)(gB + (size_t)(k + j) * g.ldb + offB[0]);
#pragma unroll
            for (int b = 0; b < NT; ++b) fb[b] = (f32x4){w[0][b], w[1][b], w[2][b], w[3][b]};
        } else {
#pragma unroll
            for (int b = 0; b < NT; ++b) fb[b] = *(gcf4)(gB + offB[b] + k);
        }
    };
    int c = wave;
#pragma nounroll
    for (; c < full_end; c += U * KW) {
        f32x4 fa[U][MT], fb[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int cu = c + u * KW;
            if (cu > full_end - 1) cu = full_end - 1;      // a short tail group re-reads the last chunk (never multiplied)
            load_chunk((cu << 4) + 4 * lg, fa[u], fb[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW >= full_end) break;
            mfma_chunk<MT, NT, BF>(acc, fa[u], fb[u]);
            if (want_colsum) {
#pragma unroll
                for (int b = 0; b < NT; ++b) csum[b] += (fb[u][b].x + fb[u][b].y) + (fb[u][b].z + fb[u][b].w);
            }
        }
    }
    // the partial last chunk of K (K % 16 != 0).  A 4-deep lane group is entirely inside K, entirely outside (it reads a valid
    // address and contributes zeros) or -- K % 4 != 0, k-contiguous A only -- straddles the end: that one group loads element by
    // element (nothing is read past the end of a row, so the last row of a matrix never reads past its allocation)
    if ((g.K & 15) && (full_end % KW) == wave) {
        const int k = (full_end << 4) + 4 * lg;
        f32x4 fa[MT], fb[NT];
        if (TA || k + 3 < g.K || k >= g.K) {
            load_chunk(k < g.K ? k : 0, fa, fb);
            if (k >= g.K) {
#pragma unroll
                for (int a = 0; a < MT; ++a) fa[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < NT; ++b) fb[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        } else {
#pragma unroll
            for (int a = 0; a < MT; ++a) fa[a] = ld_kcontig(gA + offA[TA ? 0 : a], 0, 0, true, k, g.K, false);
            if (!TB) {
                f32x4 w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[j] = (k + j < g.K) ? *(gcf4)(gB + (size_t)(k + j) * g.ldb + offB[0]) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < NT; ++b) fb[b] = (f32x4){w[0][b], w[1][b], w[2][b], w[3][b]};
            } else {
#pragma unroll
                for (int b = 0; b < NT; ++b) fb[b] = ld_kcontig(gB + offB[TB ? b : 0], 0, 0, true, k, g.K, false);
            }
        }
        mfma_chunk<MT, NT, BF>(acc, fa, fb);
        if (want_colsum) {
#pragma unroll
            for (int b = 0; b < NT; ++b) csum[b] += (fb[b].x + fb[b].y) + (fb[b].z + fb[b].w);
        }
    }

    // accumulators -> LDS tile in OUTPUT coordinates (C/D map of a 16x16 tile: column index li, row index 4 lg + r)
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = TA ? 4 * (4 * lg + r) + a : 16 * a + 4 * lg + r;
            if (!TB) {
                *(f32x4 *)&s_tile[wave][row * LDT + 4 * li] = (f32x4){acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
            } else {
#pragma unroll
                for (int b = 0; b < NT; ++b) s_tile[wave][row * LDT + 16 * b + li] = acc[a][b][r];
            }
        }
    if (want_colsum) {
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            float v = csum[b];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lg == 0) s_col[wave][TB ? 16 * b + li : 4 * li + b] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = threadIdx.x + NTH * i;
        const int r = e / TN, cidx = e - r * TN;
        const int m = m0 + r, n = n0 + cidx;
        const int off = r * LDT + cidx;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < KW; q += 4) v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
        if (g.beta != 0.f) v += g.beta * e_c[i];
        switch (g.epi) {
            case AIR_EPI_BIAS: v += e_bias[i]; break;
            case AIR_EPI_BIAS_ELU: v = elu_acc(v + e_bias[i]); break;
            case AIR_EPI_MUL_DELU: v *= (e_aux[i] > 0.f ? 1.f : e_aux[i] + 1.f); break;
            case AIR_EPI_ADD_AUX: v += e_aux[i] + e_bias[i]; break;
            case AIR_EPI_ADD_AUX_ELU: v = elu_acc(v + e_aux[i] + e_bias[i]); break;
            default: break;
        }
        if (m < g.M && n < g.N) gC[(size_t)m * g.ldc + n] = v;
    }
    if (want_colsum && threadIdx.x < TN) {
        const int n = n0 + threadIdx.x;
        if (n < g.N) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < KW; q += 4)
                v += (s_col[q][threadIdx.x] + s_col[q + 1][threadIdx.x]) + (s_col[q + 2][threadIdx.x] + s_col[q + 3][threadIdx.x]);
            gCol[n] = v;
        }
    }
}
template <int MT, int KW, bool BF, bool TA, bool TB>
__global__ __launch_bounds__(64 * KW) void gemm_wide_kernel(GemmArgs g) {
    gemm_wide_body<MT, KW, BF, TA, TB>(g, blockIdx.x);
}

// ---- the bf16 DATA path (BASELINE configs[4]) --------------------------------------------------------------------------------------
// gemm_wide_body<BF = true> only ROUNDS to bf16: every operand is still fetched as fp32 and fed to the CDNA3-form 16-deep MFMA.
// Here the operands may live in memory as bf16 -- a bf16 shadow of the flat parameter buffer (rewritten by the optimiser launch)
// and bf16 mirrors of the activations / gradients that GEMM epilogues produce (written by the producing epilogue next to the fp32
// value the non-GEMM consumers keep using) -- so an operand costs half the bytes, and the product runs on the gfx950 instruction
// v_mfma_f32_16x16x32_bf16: 32 k-slots per instruction, lane (i, lg) supplies slots 8 lg .. 8 lg + 7.  MFMA only needs A and B to
// agree on which k sits in a slot, so every loader below -- k-contiguous or interleaved along the contiguous dimension, fp32 or
// bf16 in memory -- produces "k = 32 c + 8 lg + j in slot 8 lg + j" and any combination of operand kinds multiplies correctly:
//   k-contiguous bf16 : ONE 16-byte load per lane per 32-deep chunk (8 consecutive k);
//   k-contiguous fp32 : two 16-byte loads, v_cvt_pk_bf16_f32 x4 (an operand without a mirror: LSTM state, sampled latents ...);
//   interleaved bf16  : eight 8-byte loads (row k + j, the lane's 4 columns) and a 16-bit transpose with v_perm_b32: the four
//                       values of a load go to four different MFMA tiles, exactly as in gemm_wide_body;
//   interleaved fp32  : eight 16-byte loads, converted pairwise.
// Same wave tile (16 MT x 64), same fixed-order K split over KW waves through LDS, same fused epilogues; the epilogue also writes
// the bf16 mirror of C when the descriptor names one.  fp32 accumulate, fp32 master copy of everything.

template <int MT, int KW>
struct Wide16Lds {                       // declared once per KERNEL and handed to the body: a kernel that holds several
    float tile[KW][16 * MT * (64 + 4)];  // instantiations of the body (per-problem operand kinds) must not hold several copies
    float col[KW][64];
};
template <int MT, int KW, bool TA, bool TB, bool A16, bool B16>
__device__ __forceinline__ void gemm_wide16_body(const GemmArgs &g, const Gemm16Ptrs &h, const int block_tile, Wide16Lds<MT, KW> &lds) {
    constexpr int NT = 4, TM = 16 * MT, TN = 64;
    constexpr int NTH = 64 * KW;
    constexpr int LDT = TN + 4;
    static_assert(!TA || MT == 4, "an m-contiguous A operand is read 4 rows per lane: four interleaved row tiles");
    float (&s_tile)[KW][TM * LDT] = lds.tile;
    float (&s_col)[KW][TN] = lds.col;

    const gcf gA = (gcf)g.A, gB = (gcf)g.B, gBias = (gcf)g.bias, gAux = (gcf)g.aux;
    const gch hA = (gch)h.A16, hB = (gch)h.B16;
    const gf gC = (gf)g.C, gCol = (gf)g.colsum;
    const gh_t hC = (gh_t)h.C16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int tiles_n = (g.N + TN - 1) / TN;
    const int tm = block_tile / tiles_n, tn = block_tile - tm * tiles_n;
    const int m0 = tm * TM, n0 = tn * TN;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float csum[NT] = {0.f, 0.f, 0.f, 0.f};
    const bool want_colsum = TA && (g.colsum != nullptr) && (tm == 0);

    int offA[TA ? 1 : MT], offB[TB ? NT : 1];
    if (TA) { int r = m0 + 4 * li; if (r > g.M - 4) r = g.M - 4; offA[0] = r; }
    else {
#pragma unroll
        for (int a = 0; a < MT; ++a) { int r = m0 + 16 * a + li; if (r > g.M - 1) r = g.M - 1; offA[a] = r * g.lda; }
    }
    if (!TB) { int c = n0 + 4 * li; if (c > g.N - 4) c = g.N - 4; offB[0] = c; }
    else {
#pragma unroll
        for (int b = 0; b < NT; ++b) { int c = n0 + 16 * b + li; if (c > g.N - 1) c = g.N - 1; offB[b] = c * g.ldb; }
    }

    constexpr int EPT = (TM * TN) / NTH;
    static_assert((TM * TN) % NTH == 0, "tile / threads");
    float e_bias[EPT], e_aux[EPT], e_c[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = threadIdx.x + NTH * i;
        const int r = e / TN, cidx = e - r * TN;
        int m = m0 + r, n = n0 + cidx;
        if (m > g.M - 1) m = g.M - 1;
        if (n > g.N - 1) n = g.N - 1;
        e_bias[i] = g.bias != nullptr ? gBias[n] : 0.f;
        e_aux[i] = g.epi >= AIR_EPI_MUL_DELU ? gAux[(size_t)m * g.ldaux + n] : 0.f;
        e_c[i] = g.beta != 0.f ? gC[(size_t)m * g.ldc + n] : 0.f;
    }

    // one 32-deep chunk: k = first of the lane group's eight k values, kn = number of them inside K (8 in the main loop); cs: the
    // chunk counts towards colsum -- not the last chunk a short tail group re-reads: it is never multiplied and must not be summed
    // a second time either (two chunks in flight, A16 && B16, and a K / 32 that is no multiple of 16)
    auto load_chunk = [&](int k, int kn, u32x4 (&fa)[MT], u32x4 (&fb)[NT], bool full, bool cs) {
        if (TA) {
            if (A16) {
                u32x2 w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kj = (full || j < kn) ? k + j : k;
                    w[j] = *(gcu2)(hA + (size_t)kj * g.lda + offA[0]);
                    if (!full && j >= kn) w[j] = (u32x2){0u, 0u};
                }
                fa[0] = tr16<0>(w); fa[1] = tr16<1>(w); fa[2] = tr16<2>(w); fa[3] = tr16<3>(w);
            } else {
                f32x4 w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kj = (full || j < kn) ? k + j : k;
                    w[j] = *(gcf4)(gA + (size_t)kj * g.lda + offA[0]);
                    if (!full && j >= kn) w[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                fa[0] = tr32<0>(w); fa[1] = tr32<1>(w); fa[2] = tr32<2>(w); fa[3] = tr32<3>(w);
            }
        } else {
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                if (full) {
                    if (A16) fa[a] = *(gcu4)(hA + offA[a] + k);
                    else fa[a] = pk8(*(gcf4)(gA + offA[a] + k), *(gcf4)(gA + offA[a] + k + 4));
                } else {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        v[j] = j < kn ? (A16 ? bf16_to_f32(hA[offA[a] + k + j]) : gA[offA[a] + k + j]) : 0.f;
                    fa[a] = (u32x4){pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7])};
                }
            }
        }
        if (!TB) {
            if (B16) {
                u32x2 w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kj = (full || j < kn) ? k + j : k;
                    w[j] = *(gcu2)(hB + (size_t)kj * g.ldb + offB[0]);
                    if (!full && j >= kn) w[j] = (u32x2){0u, 0u};
                }
                fb[0] = tr16<0>(w); fb[1] = tr16<1>(w); fb[2] = tr16<2>(w); fb[3] = tr16<3>(w);
                if (want_colsum && cs) { // the bias gradient sums the UNROUNDED gradient: the first row of tiles also reads the fp32 rows
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (full || j < kn) {
                            const f32x4 r = *(gcf4)(gB + (size_t)(k + j) * g.ldb + offB[0]);
                            csum[0] += r.x; csum[1] += r.y; csum[2] += r.z; csum[3] += r.w;
                        }
                    }
                }
            } else {
                f32x4 w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kj = (full || j < kn) ? k + j : k;
                    w[j] = *(gcf4)(gB + (size_t)kj * g.ldb + offB[0]);
                    if (!full && j >= kn) w[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                fb[0] = tr32<0>(w); fb[1] = tr32<1>(w); fb[2] = tr32<2>(w); fb[3] = tr32<3>(w);
                if (want_colsum && cs) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { csum[0] += w[j].x; csum[1] += w[j].y; csum[2] += w[j].z; csum[3] += w[j].w; }
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                if (full) {
                    if (B16) fb[b] = *(gcu4)(hB + offB[b] + k);
                    else fb[b] = pk8(*(gcf4)(gB + offB[b] + k), *(gcf4)(gB + offB[b] + k + 4));
                } else {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        v[j] = j < kn ? (B16 ? bf16_to_f32(hB[offB[b] + k + j]) : gB[offB[b] + k + j]) : 0.f;
                    fb[b] = (u32x4){pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7])};
                }
            }
        }
    };
    auto mma = [&](const u32x4 (&fa)[MT], const u32x4 (&fb)[NT]) {
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NT; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[a]), __builtin_bit_cast(bf16x8, fb[b]),
                                                                   acc[a][b], 0, 0, 0);
    };

    constexpr int U = (MT == 4) ? ((A16 && B16) ? 2 : 1) : 2;          // 32-deep chunks in flight per wave
    const int full_end = g.K >> 5;
    int c = wave;
#pragma nounroll
    for (; c < full_end; c += U * KW) {
        u32x4 fa[U][MT], fb[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int cu = c + u * KW;
            if (cu > full_end - 1) cu = full_end - 1;      // a short tail group re-reads the last chunk (never multiplied)
            load_chunk((cu << 5) + 8 * lg, 8, fa[u], fb[u], true, c + u * KW < full_end);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW >= full_end) break;
            mma(fa[u], fb[u]);
        }
    }
    // the partial last chunk (K % 32 != 0), element-masked, by the wave whose turn it is
    if ((g.K & 31) && (full_end % KW) == wave) {
        const int k = (full_end << 5) + 8 * lg;
        int kn = g.K - k;
        kn = kn < 0 ? 0 : (kn > 8 ? 8 : kn);
        u32x4 fa[MT], fb[NT];
        load_chunk(kn > 0 ? k : 0, kn, fa, fb, false, true);
        mma(fa, fb);
    }

#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = TA ? 4 * (4 * lg + r) + a : 16 * a + 4 * lg + r;
            if (!TB) {
                *(f32x4 *)&s_tile[wave][row * LDT + 4 * li] = (f32x4){acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
            } else {
#pragma unroll
                for (int b = 0; b < NT; ++b) s_tile[wave][row * LDT + 16 * b + li] = acc[a][b][r];
            }
        }
    if (want_colsum) {
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            float v = csum[b];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lg == 0) s_col[wave][TB ? 16 * b + li : 4 * li + b] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = threadIdx.x + NTH * i;
        const int r = e / TN, cidx = e - r * TN;
        const int m = m0 + r, n = n0 + cidx;
        const int off = r * LDT + cidx;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < KW; q += 4) v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
        if (g.beta != 0.f) v += g.beta * e_c[i];
        switch (g.epi) {
            case AIR_EPI_BIAS: v += e_bias[i]; break;
            case AIR_EPI_BIAS_ELU: v = elu_acc(v + e_bias[i]); break;
            case AIR_EPI_MUL_DELU: v *= (e_aux[i] > 0.f ? 1.f : e_aux[i] + 1.f); break;
            case AIR_EPI_ADD_AUX: v += e_aux[i] + e_bias[i]; break;
            case AIR_EPI_ADD_AUX_ELU: v = elu_acc(v + e_aux[i] + e_bias[i]); break;
            default: break;
        }
        if (m < g.M && n < g.N) {
            gC[(size_t)m * g.ldc + n] = v;
            if (hC) hC[(size_t)m * g.ldc + n] = bf16_bits(v);
        }
    }
    if (want_colsum && threadIdx.x < TN) {
        const int n = n0 + threadIdx.x;
        if (n < g.N) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < KW; q += 4)
                v += (s_col[q][threadIdx.x] + s_col[q + 1][threadIdx.x]) + (s_col[q + 2][threadIdx.x] + s_col[q + 3][threadIdx.x]);
            gCol[n] = v;
        }
    }
}
template <int MT, int KW, bool TA, bool TB, bool A16, bool B16>
__global__ __launch_bounds__(64 * KW) void gemm_wide16_kernel(GemmArgs g, Gemm16Ptrs h) {
    __shared__ Wide16Lds<MT, KW> lds;
    gemm_wide16_body<MT, KW, TA, TB, A16, B16>(g, h, blockIdx.x, lds);
}

// Several independent GEMMs in ONE launch (the step is launch/latency bound: a dW / dX pair, or the two heads that
// read the same hidden state, cost one dispatch instead of two).  Problem p owns blocks [tile_start[p], tile_start[p+1]).
#define AIR_GEMM_GROUP_MAX 8
struct GroupArgs {
    GemmArgs g[AIR_GEMM_GROUP_MAX];
    int tile_start[AIR_GEMM_GROUP_MAX + 1];
    int count;
    int xcd_map;          // wide-tile launches: blockIdx -> tile through xcd_contiguous_tile
    unsigned sk_mask;     // bit p: problem p is a short-K weight gradient on the streaming body (shortk_dw_body); its range = its workgroups
};
// The slot dispatch of every grouped kernel: find the problem p that owns workgroup VB_ (wave-uniform, hence the readfirstlane) and
// run CASE_(slot) for it -- CASE_ is the kernel's one-line call of its body with a CONSTANT slot index.  (The two halves are macros
// of their own for the one kernel that needs p between them.)
//   * One specialised copy of the body per descriptor slot: with a CONSTANT index the descriptor is read straight from the kernarg
//     SGPRs like a single-GEMM launch (94 VGPRs).  A dynamic index (or a descriptor copied through memory) costs +100 VGPRs and
//     halves the occupancy of exactly the launches that have the most workgroups.
//   * The tile kernels pass blockIdx.y as the split: it is always 0 there, but passing it instead of a literal 0 keeps hipcc from
//     restructuring the K loop around a known start, which doubles the live registers (94 -> 194 VGPRs, measured).
//   * ONE instantiation of the body per slot, a fold / epilogue choice being a wave-uniform run-time flag of it: two instantiations
//     would each bring their own static LDS tile and halve the workgroups a CU holds.
// A macro on purpose.  The same dispatch as a __forceinline__ template that calls a generic lambda with an integral_constant slot
// (group struct captured or not) was compiled and compared per kernel: +9..12 SGPRs on every gemm_grouped_kernel /
// gemm_grouped_opt_kernel, and 98-161 SGPR spills (48-62 -> 104-106 SGPRs, occupancy moved on two) on all 16
// gemm_grouped_wide16_kernel instantiations.  The macro expands to the tokens that used to be written out in each kernel and
// leaves the resource usage of every kernel of this file as it was (profiles/gemm_split_resources.txt).
#define AIR_GROUP_LOCATE(P_, GA_, VB_)                                                                                           \
    int P_ = 0;                                                                                                                  \
    _Pragma("unroll")                                                                                                            \
    for (int i = 1; i < AIR_GEMM_GROUP_MAX; ++i)                                                                                 \
        if (i < GA_.count && VB_ >= GA_.tile_start[i]) P_ = i;                                                                   \
    P_ = __builtin_amdgcn_readfirstlane(P_)
#define AIR_GROUP_SWITCH(P_, CASE_)                                                                                              \
    switch (P_) {                                                                                                                \
        case 0: CASE_(0); break;                                                                                                 \
        case 1: CASE_(1); break;                                                                                                 \
        case 2: CASE_(2); break;                                                                                                 \
        case 3: CASE_(3); break;                                                                                                 \
        case 4: CASE_(4); break;                                                                                                 \
        case 5: CASE_(5); break;                                                                                                 \
        case 6: CASE_(6); break;                                                                                                 \
        default: CASE_(7); break;                                                                                                \
    }
#define AIR_GROUP_DISPATCH(GA_, VB_, CASE_)                                                                                      \
    do {                                                                                                                         \
        AIR_GROUP_LOCATE(p, GA_, VB_);                                                                                           \
        AIR_GROUP_SWITCH(p, CASE_);                                                                                              \
    } while (0)
template <int MT, int NT, int KW, bool BF>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_grouped_kernel(GroupArgs ga) {
#define AIR_GG_CASE(I_) gemm_body<MT, NT, KW, BF>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y)
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_GG_CASE);
#undef AIR_GG_CASE
}

// gemm_grouped_kernel<1, 1, 16, false> for a launch of few long-K NT problems (the d h_{-1} / d enc_out pair behind the BPTT: 2 x 64
// tiles, K = 1024, each tile's CU taking in 128 KB of operands beside 128 idle CUs): problem i owns 8 rows (bit 2 i of own8) and 8
// columns (bit 2 i + 1) of each MFMA tile instead of 16, on two or four times the workgroups; same bits (gemm_body, HALF).
__global__ __launch_bounds__(1024) void gemm_grouped_longk_half_kernel(GroupArgs ga, unsigned own8) {
#define AIR_GH_CASE(I_)                                                                                                              \
    gemm_body<1, 1, 16, false, false, false, false, false, true>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y, AproArgs(),  \
                                                                 nullptr, nullptr, false, nullptr, nullptr, false,                  \
                                                                 ((own8 >> (2 * I_)) & 1u) ? 8 : 16, ((own8 >> (2 * I_ + 1)) & 1u) ? 8 : 16)
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_GH_CASE);
#undef AIR_GH_CASE
}

// gemm_grouped_kernel<1, 1, 16> whose problems read their A rows through the feeder's index (GatherArgs): the first launch of a
// latency-regime train step with an HBM-resident dataset attached (air_gemm_grouped_gather)
__global__ __launch_bounds__(1024) void gemm_grouped_gather_kernel(GroupArgs ga, GatherArgs gt) {
#define AIR_GG_CASE(I_)                                                                                                             \
    gemm_body<1, 1, 16, false, false, false, false, true>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y, AproArgs(), nullptr, \
                                                          nullptr, false, nullptr, &gt, cp)
    AIR_GROUP_LOCATE(p, ga, (int)blockIdx.x);
    const bool cp = (gt.copy_mask >> p) & 1u;
    AIR_GROUP_SWITCH(p, AIR_GG_CASE);
#undef AIR_GG_CASE
}

// gemm_grouped_kernel whose weight-gradient problems (fold_mask) apply the centred-RMSProp update to the elements they finish, with
// rider workgroups (blockIdx >= tiles) updating the slices earlier launches left final and advancing the step counters
template <int MT, int NT, int KW, bool BF>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_grouped_opt_kernel(GroupArgs ga, OptFold opt) {
    AIR_OPT_RIDERS(opt);
#define AIR_OPT_CASE(I_)                                                                                                          \
    gemm_body<MT, NT, KW, BF, false, true>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y, AproArgs(), nullptr, &opt,  \
                                           ((opt.fold_mask >> I_) & 1u) != 0)
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_OPT_CASE);
#undef AIR_OPT_CASE
}

// ---- short-K weight gradients of the wide first layers (latency regime: dW[M, N] = X^T . dY with K = batch rows <= 64, M = 2500 /
// 10000 pixels, N <= 256): thousands of output tiles each fed by ONE 16-deep chunk per wave.  On the tile kernels every workgroup is
// a chain of one cold operand round trip, an LDS reduction of four single-chunk partials, a barrier and the epilogue -- 2500 such
// workgroups in three resident rounds: 10-17 us beside a 5 us critical path, 30 us where the update rides (configs[3]).  Here the
// product STREAMS: a wave keeps the whole dY[K, 64 columns] operand of its column quarter in registers (K <= 64: sixteen float4) and
// walks 16-row slabs of the output grid-stride -- four dword loads per chunk of X^T, sixteen MFMAs per chunk, the accumulators
// stored (and, folded, updated) straight from the MFMA layout; the next slab's operand is requested before the current one is
// multiplied.  No LDS, no barrier, no K split (one accumulation chain per element: a fixed order).
template <bool OPT>
__device__ __forceinline__ void shortk_dw_body(const GemmArgs &g, const int vb, const int vg, const OptFold *opt, const bool fold) {
    const gcf gA = (gcf)g.A, gB = (gcf)g.B;
    const gf gC = (gf)g.C, gCol = (gf)g.colsum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int n_base = 64 * wave;
    if (n_base >= g.N) return;                                   // (N % 64 == 0: whole quarters; no barrier anywhere below)
    const int nch = g.K >> 4;                                    // K % 16 == 0, K <= 64
    f32x4 fb[4][4];                                              // fb[c][t][j] = dY[16c + 4lg + j, n_base + 16t + li]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            fb[c][t] = c < nch ? ld_kstrided_full(gB, g.ldb, n_base + 16 * t + li, (c << 4) + 4 * lg) : (f32x4){0.f, 0.f, 0.f, 0.f};
    float o_lr0 = 0.f;
    if (OPT && fold) o_lr0 = ((gcf)opt->lr_dev)[0];
    if (gCol != nullptr && vb == 0) {                            // the bias gradient: column sums of dY, by the first workgroup
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) v += (fb[c][t].x + fb[c][t].y) + (fb[c][t].z + fb[c][t].w);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lg == 0) {
                const int n = n_base + 16 * t + li;
                gCol[n] = v;
                if (OPT && fold) {
                    const size_t idx = (size_t)((gCol + n) - (gf)opt->g0);
                    const float lr = idx < opt->n_model ? o_lr0 : o_lr0 * opt->lr_mult_tail;
                    float pv = ((gf)opt->p)[idx], a = ((gf)opt->ms)[idx], b = ((gf)opt->mg)[idx], cmo = ((gf)opt->mom)[idx];
                    rmsprop_elem(pv, v, a, b, cmo, lr, opt->decay, opt->momentum, opt->eps, opt->gscale);
                    ((gf)opt->ms)[idx] = a; ((gf)opt->mg)[idx] = b; ((gf)opt->mom)[idx] = cmo; ((gf)opt->p)[idx] = pv;
                }
            }
        }
    }
    const int tiles_m = (g.M + 15) >> 4;
    int mt = vb;
    if (mt >= tiles_m) return;
    f32x4 fa[4];
    {
        int m = (mt << 4) + li; if (m > g.M - 1) m = g.M - 1;
#pragma unroll
        for (int c = 0; c < 4; ++c) fa[c] = c < nch ? ld_kstrided_full(gA, g.lda, m, (c << 4) + 4 * lg) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma nounroll
    for (; mt < tiles_m; mt += vg) {
        f32x4 fn[4];
        {   // the next slab's operand, requested before this one is multiplied (clamped: a slab past the end is never used)
            int mn = ((mt + vg) << 4) + li; if (mn > g.M - 1) mn = g.M - 1;
#pragma unroll
            for (int c = 0; c < 4; ++c) fn[c] = c < nch ? ld_kstrided_full(gA, g.lda, mn, (c << 4) + 4 * lg) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const int mrow0 = (mt << 4) + 4 * lg;
        // folded update: parameter and slots of this lane's 16 elements, requested before the product
        f32x4 o_p[4], o_ms[4], o_mg[4], o_mom[4];               // [t][r]
#pragma unroll
        for (int t = 0; t < 4; ++t) { o_p[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; o_ms[t] = o_p[t]; o_mg[t] = o_p[t]; o_mom[t] = o_p[t]; }
        if (OPT && fold) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int mr = mrow0 + r; if (mr > g.M - 1) mr = g.M - 1;
                const size_t idx0 = (size_t)((gC + (size_t)mr * g.ldc + n_base + li) - (gf)opt->g0);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    o_p[t][r] = ((gf)opt->p)[idx0 + 16 * t]; o_ms[t][r] = ((gf)opt->ms)[idx0 + 16 * t];
                    o_mg[t][r] = ((gf)opt->mg)[idx0 + 16 * t]; o_mom[t][r] = ((gf)opt->mom)[idx0 + 16 * t];
                }
            }
        }
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[c][j], fb[c][t][j], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mr = mrow0 + r;
                if (mr < g.M) {
                    const size_t off = (size_t)mr * g.ldc + n_base + 16 * t + li;
                    const float v = acc[t][r];
                    gC[off] = v;
                    if (OPT && fold) {
                        const size_t idx = (size_t)((gC + off) - (gf)opt->g0);
                        const float lr = idx < opt->n_model ? o_lr0 : o_lr0 * opt->lr_mult_tail;
                        float pv = o_p[t][r], a = o_ms[t][r], b = o_mg[t][r], cmo = o_mom[t][r];
                        rmsprop_elem(pv, v, a, b, cmo, lr, opt->decay, opt->momentum, opt->eps, opt->gscale);
                        ((gf)opt->ms)[idx] = a; ((gf)opt->mg)[idx] = b; ((gf)opt->mom)[idx] = cmo; ((gf)opt->p)[idx] = pv;
                    }
                }
            }
#pragma unroll
        for (int c = 0; c < 4; ++c) fa[c] = fn[c];
    }
}
// what the streaming body takes (host side): an fp32 TN weight gradient with no epilogue, K in {16, 32, 48, 64}, N a multiple of 64 up
// to 256, and at least AIR_GEMM_SHORTK_MIN_M (4096) output rows.  Measured (profiles/r05_shortk_dw_ab.txt): at 10000 rows (configs[3])
// the launch beside the decoder's dX drops from 16.6 to 10.3 us and the closing launch with the folded update from 30.4 to 25.5 us;
// at 2500 rows (configs[1]: 157 slabs, ONE per workgroup, so the register-resident dY operand is loaded for a single slab) the
// closing launch is SLOWER (12.0 against 9.7 us) -- hence the row threshold.  The same rule in every entry point (a problem's
// product must not depend on which launch carries it: the folded and the unfolded plan are bit-identical).  AIR_GEMM_SHORTK=0: never.
static inline bool shortk_eligible(const AirGemmDesc &d) {
    static const int on = getenv("AIR_GEMM_SHORTK") ? atoi(getenv("AIR_GEMM_SHORTK")) : 1;
    static const int min_m = getenv("AIR_GEMM_SHORTK_MIN_M") ? atoi(getenv("AIR_GEMM_SHORTK_MIN_M")) : 4096;
    return on && d.ta && !d.tb && d.precision == AIR_PREC_F32 && d.K >= 16 && d.K <= 64 && d.K % 16 == 0 && d.N >= 64 && d.N <= 256 &&
           d.N % 64 == 0 && d.M >= min_m && d.epilogue == AIR_EPI_NONE && d.beta == 0.f && !d.A2 && !d.C16 && !d.bias;
}
static inline int shortk_workgroups(int M) {
    static const int cap = getenv("AIR_GEMM_SHORTK_WGS") ? atoi(getenv("AIR_GEMM_SHORTK_WGS")) : 384;
    const int t = air_cdiv(M, 16);
    return t < cap ? t : (cap < 1 ? 1 : cap);
}

// gemm_grouped_kernel (4-wave tiles) with short-K weight gradients of ga.sk_mask on the streaming body
template <int MT, int NT>
__global__ __launch_bounds__(256) void gemm_grouped_sk_kernel(GroupArgs ga) {
#define AIR_SK_CASE(I_)                                                                                                        \
    do {                                                                                                                       \
        if ((ga.sk_mask >> I_) & 1u)                                                                                           \
            shortk_dw_body<false>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], ga.tile_start[I_ + 1] - ga.tile_start[I_], nullptr, false); \
        else gemm_body<MT, NT, 4, false>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y);                           \
    } while (0)
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_SK_CASE);
#undef AIR_SK_CASE
}
// gemm_grouped_opt_kernel's counterpart for launches whose problems are ALL short-K weight gradients (the closing launch of the
// latency-regime step: the first layer over the pixels of obs): a folded problem updates its elements from the MFMA layout
__global__ __launch_bounds__(256) void gemm_grouped_opt_sk_kernel(GroupArgs ga, OptFold opt) {
    AIR_OPT_RIDERS(opt);
#define AIR_SK_CASE(I_)                                                                                                        \
    shortk_dw_body<true>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], ga.tile_start[I_ + 1] - ga.tile_start[I_], &opt,        \
                         ((opt.fold_mask >> I_) & 1u) != 0)
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_SK_CASE);
#undef AIR_SK_CASE
}

// gemm_grouped_kernel whose problem(s) of `gb.mask` finish a Gaussian head's backward in their epilogue, with up to two rider
// workgroups behind the tiles: the NVIL objective (nvil_device.h; nv.imp == NULL: none) and the sum of the head's KL shares
// (engine_device.h kl_parts_sum; kp.n_parts == 0: none) -- what air_gauss_sample_bwd_nvil did as a launch of its own
template <int MT, int NT, int KW, bool BF>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_grouped_gb_kernel(GroupArgs ga, GaussEpi gb, NvilArgs nv, KlParts kp, int tiles,
                                                                                  int kl_rows) {
    if ((int)blockIdx.x >= tiles) {
        const int r = (int)blockIdx.x - tiles;
        if (r == 0 && nv.imp) nvil_body(nv);
        else kl_parts_sum(kp, kl_rows);
        return;
    }
#define AIR_GB_CASE(I_)                                                                                                                  \
    gemm_body<MT, NT, KW, BF, false, false, true>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y, AproArgs(), nullptr, nullptr,  \
                                                  ((gb.mask >> I_) & 1u) != 0, &gb)
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_GB_CASE);
#undef AIR_GB_CASE
}

struct C16Ptrs { void *p[AIR_GEMM_GROUP_MAX]; };
template <int MT, int NT, int KW>
__global__ __launch_bounds__(KW == 1 ? 256 : 64 * KW) void gemm_grouped_c16_kernel(GroupArgs ga, C16Ptrs c16) {
#define AIR_C16_CASE(I_) gemm_body<MT, NT, KW, true>(ga.g[I_], (int)blockIdx.x - ga.tile_start[I_], blockIdx.y, AproArgs(), c16.p[I_])
    AIR_GROUP_DISPATCH(ga, (int)blockIdx.x, AIR_C16_CASE);
#undef AIR_C16_CASE
}

// consecutive workgroup ids go to different XCDs (each with its own L2): give every XCD a CONTIGUOUS range of tiles -- same
// problem, same row slab, neighbouring column slabs -- so that an operand slab is pulled into one L2, not into all eight
__device__ __forceinline__ int xcd_contiguous_tile(int b, int G) {
    const int full = G >> 3, rem = G & 7, x = b & 7, i = b >> 3;
    return x * full + (x < rem ? x : rem) + i;
}
template <int MT, int KW, bool BF, bool TA, bool TB>
__global__ __launch_bounds__(64 * KW) void gemm_grouped_wide_kernel(GroupArgs ga) {
    const int vb = ga.xcd_map ? xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
#define AIR_WIDE_CASE(I_) gemm_wide_body<MT, KW, BF, TA, TB>(ga.g[I_], vb - ga.tile_start[I_])
    AIR_GROUP_DISPATCH(ga, vb, AIR_WIDE_CASE);
#undef AIR_WIDE_CASE
}

struct GroupArgs16 {
    GemmArgs g[AIR_GEMM_GROUP_MAX];
    Gemm16Ptrs h[AIR_GEMM_GROUP_MAX];
    int tile_start[AIR_GEMM_GROUP_MAX + 1];
    int count;
    int xcd_map;
};
template <int MT, int KW, bool TA, bool TB, bool A16, bool B16>
__global__ __launch_bounds__(64 * KW) void gemm_grouped_wide16_kernel(GroupArgs16 ga) {
    __shared__ Wide16Lds<MT, KW> lds;
    const int vb = ga.xcd_map ? xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
#define AIR_WIDE16_CASE(I_) gemm_wide16_body<MT, KW, TA, TB, A16, B16>(ga.g[I_], ga.h[I_], vb - ga.tile_start[I_], lds)
    AIR_GROUP_DISPATCH(ga, vb, AIR_WIDE16_CASE);
#undef AIR_WIDE16_CASE
}

// All weight gradients of a step in ONE launch: up to 24 all-TN problems (a dynamic, wave-uniform descriptor index: scalar
// loads from the kernel-argument segment).  With every long-K and short-K tile in the same grid -- long ones first -- the CUs
// that finish early keep pulling short tiles instead of idling until the launch ends (two launches of 8: 72 + 69 us in fp32 at
// batch 1024 with 184 and 408 tiles on 256 CUs).
#define AIR_GEMM_BIG_GROUP_MAX 24
struct BigGroupArgs {
    GemmArgs g[AIR_GEMM_BIG_GROUP_MAX];
    int tile_start[AIR_GEMM_BIG_GROUP_MAX + 1];
    int count;
    int xcd_map;          // 0: none, 1: XCD-contiguous tiles within each problem, 2: over the whole grid
    unsigned small_mask;  // bit p: problem p is not wide-tile eligible (one to three rows, one column ...): 16x16 tiles, gemm_body
};
// the same within ONE problem's range of workgroup ids [s, e): the problem keeps its place in the dispatch order (long-K problems
// first), and the workgroups of it that land on one XCD (ids congruent mod 8) get a contiguous run of its tiles
__device__ __forceinline__ int xcd_contiguous_tile_in_range(int b, int s, int e) {
    const int x = b & 7;
    int start = 0, first_x = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const int f = s + ((y - s) & 7);                    // first id >= s on XCD y
        const int cnt = f < e ? ((e - 1 - f) >> 3) + 1 : 0;
        if (y < x) start += cnt;
        if (y == x) first_x = f;
    }
    return s + start + ((b - first_x) >> 3);
}
// (the odd-shaped rest of the weight gradients -- eight long-K reductions with one to three rows or a single column -- rides in
//  the same grid on the 16x16-tile body with the same 8 K-splitting waves: a launch of their own cost 14.5 us at batch 1024)
template <int MT, int KW, bool BF>
__global__ __launch_bounds__(64 * KW) void gemm_big_group_wide_tn_kernel(BigGroupArgs ga) {
    const int b = ga.xcd_map == 2 ? xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    int p = 0;
    for (int i = 1; i < ga.count; ++i)
        if (b >= ga.tile_start[i]) p = i;
    p = __builtin_amdgcn_readfirstlane(p);
    const int s0 = ga.tile_start[p];
    if ((ga.small_mask >> p) & 1u) {
        gemm_body<1, 1, KW, BF>(ga.g[p], b - s0, 0);
        return;
    }
    const int vb = ga.xcd_map == 1 ? xcd_contiguous_tile_in_range(b, s0, ga.tile_start[p + 1]) : b;
    gemm_wide_body<MT, KW, BF, true, false>(ga.g[p], vb - s0);
}

// bf16 data path: the same launch with the operands' bf16 mirrors (weight gradients: A = an activation, B = a gradient, both
// interleaved reads); the odd-shaped members keep the fp32-fetch small-tile body
struct BigGroupArgs16 {
    GemmArgs g[AIR_GEMM_BIG_GROUP_MAX];
    Gemm16Ptrs h[AIR_GEMM_BIG_GROUP_MAX];
    int tile_start[AIR_GEMM_BIG_GROUP_MAX + 1];
    int count;
    int xcd_map;
    unsigned small_mask;
};
// (the operand kinds are per PROBLEM here -- a weight-gradient launch mixes activations with and without a mirror -- chosen by a
//  wave-uniform branch between the four instantiations of the body)
template <int MT, int KW>
__global__ __launch_bounds__(64 * KW) void gemm_big_group_wide16_tn_kernel(BigGroupArgs16 ga) {
    __shared__ Wide16Lds<MT, KW> lds;
    const int b = ga.xcd_map == 2 ? xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    int p = 0;
    for (int i = 1; i < ga.count; ++i)
        if (b >= ga.tile_start[i]) p = i;
    p = __builtin_amdgcn_readfirstlane(p);
    const int s0 = ga.tile_start[p];
    if ((ga.small_mask >> p) & 1u) {
        gemm_body<1, 1, KW, true>(ga.g[p], b - s0, 0);
        return;
    }
    const int vb = ga.xcd_map == 1 ? xcd_contiguous_tile_in_range(b, s0, ga.tile_start[p + 1]) : b;
    const bool a16 = ga.h[p].A16 != nullptr, b16 = ga.h[p].B16 != nullptr;
    if (a16 && b16) gemm_wide16_body<MT, KW, true, false, true, true>(ga.g[p], ga.h[p], vb - s0, lds);
    else if (a16) gemm_wide16_body<MT, KW, true, false, true, false>(ga.g[p], ga.h[p], vb - s0, lds);
    else if (b16) gemm_wide16_body<MT, KW, true, false, false, true>(ga.g[p], ga.h[p], vb - s0, lds);
    else gemm_wide16_body<MT, KW, true, false, false, false>(ga.g[p], ga.h[p], vb - s0, lds);
}

// sums the S split-K slabs in fixed order and applies the epilogue
__global__ __launch_bounds__(256) void gemm_splitk_epilogue_kernel(GemmArgs g) {
    const size_t total = (size_t)g.M * g.N;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int m = (int)(e / g.N), n = (int)(e - (size_t)m * g.N);
        float v = 0.f;
        for (int s = 0; s < g.S; ++s) v += g.ws[(size_t)s * total + e];
        g.C[(size_t)m * g.ldc + n] = apply_epilogue(v, m, n, g);
    }
}

template <int MT, int NT, int KW, bool BF>
static int launch_gemm(const GemmArgs &g, hipStream_t st) {
    constexpr int TM = 16 * MT, TN = 16 * NT * ((KW == 1) ? 4 : 1);
    const int tiles = air_cdiv(g.M, TM) * air_cdiv(g.N, TN);
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<MT, NT, KW, BF>), dim3(tiles, g.S), dim3(KW == 1 ? 256 : 64 * KW), 0, st, g);
    AIR_LAUNCH_CHECK();
    if (g.S > 1) {
        const size_t total = (size_t)g.M * g.N;
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(gemm_splitk_epilogue_kernel, dim3(blocks), dim3(256), 0, st, g);
        AIR_LAUNCH_CHECK();
    }
    return AIR_OK;
}

extern "C" size_t air_gemm_workspace_bytes(int M, int N, int K) {
    (void)K;
    if (M <= 0 || N <= 0) return 0;
    return (size_t)16 * (size_t)M * (size_t)N * sizeof(float);     // up to 16 split-K slabs
}

// WHICH kernel air_gemm / air_gemm_bf16 run (M, N, K > 0): the decision gemm_dispatch consumes and air_gemm_form returns.
// tile shape: few rows -> narrow tiles + intra-workgroup split-K; many tiles -> one tile per wave
static void gemm_single_form(int M, int N, int K, bool colsum, bool ws, size_t ws_bytes, AirGemmForm &f) {
    memset(&f, 0, sizeof f);
    f.family = AIR_GEMM_FAM_TILE;
    const int chunks = (K + 15) / 16;
    const long tiles22 = (long)air_cdiv(M, 32) * air_cdiv(N, 32);
    if (tiles22 >= 2048) {
        f.MT = 2; f.NT = 2; f.KW = 1; f.tile = 32; f.S = 1; f.chunks_per_split = chunks;
        f.workgroups = air_cdiv(M, 32) * air_cdiv(N, 128); f.threads = 256;
        return;
    }
    // latency regime (the whole problem fits a fraction of the chip): 16x16 tiles, one per workgroup, 4 waves split K,
    // 8 chunks in flight -- every wave does one or two memory round trips whatever the shape
    const long tiles = (long)air_cdiv(M, 16) * air_cdiv(N, 16);
    int S = 1;
    // cross-workgroup split-K costs a second (epilogue) launch, ~4.5 us on this part: only worth it for long K
    if (!colsum && ws && chunks >= 64) {
        long want = 1024 / (tiles > 0 ? tiles : 1);                      // aim for ~4 workgroups per CU
        long max_by_k = chunks / 16;                                     // >= 4 chunks per wave per split
        long max_by_ws = (long)(ws_bytes / ((size_t)M * N * sizeof(float)));
        long s = want;
        if (s > max_by_k) s = max_by_k;
        if (s > max_by_ws) s = max_by_ws;
        if (s > 16) s = 16;
        if (s >= 2) S = (int)s;
    }
    f.MT = 1; f.NT = 1; f.KW = 4; f.tile = 16;
    f.chunks_per_split = (chunks + S - 1) / S;
    f.S = (chunks + f.chunks_per_split - 1) / f.chunks_per_split;       // drop empty tail splits
    f.workgroups = (int)tiles; f.threads = 256;
}
extern "C" int air_gemm_form(int M, int N, int K, int colsum, size_t ws_bytes, AirGemmForm *out) {
    AIR_REQUIRE(out, AIR_E_NULL);
    AIR_REQUIRE(M > 0 && N > 0 && K > 0, AIR_E_SHAPE);
    gemm_single_form(M, N, K, colsum != 0, ws_bytes > 0, ws_bytes, *out);
    return AIR_OK;
}

template <bool BF>
static int gemm_dispatch(int ta, int tb, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                         float *C, int ldc, const float *bias, int epilogue, const float *aux, int ldaux, float beta,
                         float *colsum, void *ws, size_t ws_bytes, void *stream) {
    AIR_REQUIRE(A && B && C, AIR_E_NULL);
    AIR_REQUIRE(M > 0 && N > 0 && K > 0, AIR_E_SHAPE);
    AIR_REQUIRE(lda >= (ta ? M : K) && ldb >= (tb ? K : N) && ldc >= N, AIR_E_SHAPE);
    AIR_REQUIRE(epilogue >= AIR_EPI_NONE && epilogue <= AIR_EPI_ADD_AUX_ELU, AIR_E_UNSUPPORTED);
    if (epilogue == AIR_EPI_BIAS || epilogue == AIR_EPI_BIAS_ELU) AIR_REQUIRE(bias, AIR_E_NULL);
    if (epilogue >= AIR_EPI_MUL_DELU) AIR_REQUIRE(aux && ldaux >= N, AIR_E_NULL);
    AIR_REQUIRE(!colsum || ta, AIR_E_UNSUPPORTED);

    GemmArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.aux = aux; g.colsum = colsum; g.ws = (float *)ws;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux;
    g.ta = ta ? 1 : 0; g.tb = tb ? 1 : 0; g.epi = epilogue; g.beta = beta;
    g.vecA = (!ta && (lda % 4 == 0) && air_aligned16(A)) ? 1 : 0;
    g.vecB = (tb && (ldb % 4 == 0) && air_aligned16(B)) ? 1 : 0;

    AirGemmForm f;
    gemm_single_form(M, N, K, colsum != nullptr, ws != nullptr, ws_bytes, f);
    g.S = f.S; g.chunks_per_split = f.chunks_per_split;
    hipStream_t st = air_stream(stream);
    if (f.KW == 1) return launch_gemm<2, 2, 1, BF>(g, st);
    return launch_gemm<1, 1, 4, BF>(g, st);
}

extern "C" int air_gemm(int ta, int tb, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                        float *C, int ldc, const float *bias, int epilogue, const float *aux, int ldaux, float beta,
                        float *colsum, void *ws, size_t ws_bytes, void *stream) {
    return gemm_dispatch<false>(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, epilogue, aux, ldaux, beta, colsum, ws,
                                ws_bytes, stream);
}
extern "C" int air_gemm_bf16(int ta, int tb, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                             float *C, int ldc, const float *bias, int epilogue, const float *aux, int ldaux, float beta,
                             float *colsum, void *ws, size_t ws_bytes, void *stream) {
    return gemm_dispatch<true>(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, epilogue, aux, ldaux, beta, colsum, ws,
                               ws_bytes, stream);
}

static int fill_gemm_args(GemmArgs &g, const AirGemmDesc &d) {
    AIR_REQUIRE(d.A && d.B && d.C, AIR_E_NULL);
    AIR_REQUIRE(d.M > 0 && d.N > 0 && d.K > 0, AIR_E_SHAPE);
    AIR_REQUIRE(d.lda >= (d.ta ? d.M : d.K) && d.ldb >= (d.tb ? d.K : d.N) && d.ldc >= d.N, AIR_E_SHAPE);
    AIR_REQUIRE(d.epilogue >= AIR_EPI_NONE && d.epilogue <= AIR_EPI_ADD_AUX_ELU, AIR_E_UNSUPPORTED);
    if (d.epilogue == AIR_EPI_BIAS || d.epilogue == AIR_EPI_BIAS_ELU) AIR_REQUIRE(d.bias, AIR_E_NULL);
    if (d.epilogue >= AIR_EPI_MUL_DELU) AIR_REQUIRE(d.aux && d.ldaux >= d.N, AIR_E_NULL);
    AIR_REQUIRE(!d.colsum || d.ta, AIR_E_UNSUPPORTED);
    if (d.A2) {       // the A prologue: k-contiguous A, both slabs and the bias readable with the same 16-byte loads, K % 16 == 0
        AIR_REQUIRE(!d.ta && d.a_bias && (d.K % 16 == 0) && (d.lda % 4 == 0), AIR_E_UNSUPPORTED);
        AIR_REQUIRE(air_aligned16(d.A) && air_aligned16(d.A2) && air_aligned16(d.a_bias) && (!d.a_out || air_aligned16(d.a_out)),
                    AIR_E_ALIGN);
    }
    g.A = d.A; g.B = d.B; g.C = d.C; g.bias = d.bias; g.aux = d.aux; g.colsum = d.colsum; g.ws = nullptr;
    g.M = d.M; g.N = d.N; g.K = d.K; g.lda = d.lda; g.ldb = d.ldb; g.ldc = d.ldc; g.ldaux = d.ldaux;
    g.ta = d.ta ? 1 : 0; g.tb = d.tb ? 1 : 0; g.epi = d.epilogue; g.beta = d.beta;
    g.vecA = (!d.ta && (d.lda % 4 == 0) && air_aligned16(d.A)) ? 1 : 0;
    g.vecB = (d.tb && (d.ldb % 4 == 0) && air_aligned16(d.B)) ? 1 : 0;
    g.S = 1; g.chunks_per_split = (d.K + 15) / 16;
    return AIR_OK;
}

// ---- group planning: what every grouped entry point does with its descriptors, written once (a problem's product must not
// depend on which launch carries it, see shortk_eligible) -------------------------------------------------------------------------
// Workgroup ranges: problem i owns [tile_start[i], tile_start[i + 1]); tiles_of(i, d) is the number of workgroups it gets, or an
// AIR_E_* (< 0) that refuses it.  The tail is padded with the total.  Returns the total, or that refusal.
template <class GA, class Tiles>
static int group_tile_starts(GA &ga, const AirGemmDesc *descs, int count, Tiles tiles_of) {
    constexpr int MAX = (int)(sizeof(ga.g) / sizeof(ga.g[0]));
    int tiles = 0;
    for (int i = 0; i < count; ++i) {
        ga.tile_start[i] = tiles;
        const int t = tiles_of(i, descs[i]);
        if (t < 0) return t;
        tiles += t;
    }
    for (int i = count; i <= MAX; ++i) ga.tile_start[i] = tiles;
    return tiles;
}
static int accept_any(int, const AirGemmDesc &) { return AIR_OK; }
// Fills a GroupArgs / BigGroupArgs from `count` descriptors.  Per problem, in order: accept(i, d) -- the entry point's own refusal
// of the problem, AIR_OK to take it --, fill_gemm_args, tiles_of(i, d) as above: the first error in that order is returned, as the
// entry points did when each wrote this loop out.  Unused slots repeat problem 0 (every slot of the kernel's switch reads a valid
// descriptor), the workgroup map and the streaming mask start cleared.  *total = workgroups of the launch.
template <class GA, class Accept, class Tiles>
static int fill_group(GA &ga, const AirGemmDesc *descs, int count, Accept accept, Tiles tiles_of, int *total) {
    constexpr int MAX = (int)(sizeof(ga.g) / sizeof(ga.g[0]));
    const int tiles = group_tile_starts(ga, descs, count, [&](int i, const AirGemmDesc &d) {
        int st = accept(i, d);
        if (st == AIR_OK) st = fill_gemm_args(ga.g[i], d);
        return st ? st : tiles_of(i, d);
    });
    if (tiles < 0) return tiles;
    for (int i = count; i < MAX; ++i) ga.g[i] = ga.g[0];
    ga.count = count;
    ga.xcd_map = 0;
    if constexpr (std::is_same<GA, GroupArgs>::value) ga.sk_mask = 0;
    *total = tiles;
    return AIR_OK;
}
// the bf16-data-path sibling (GroupArgs16 / BigGroupArgs16) of a filled group: the same problems and workgroup ranges, plus the
// operand / result mirrors that mirrors_of(j) chooses for problem j
template <class GA16, class GA, class Mirrors>
static void group_to16(GA16 &g16, const GA &ga, Mirrors mirrors_of) {
    constexpr int MAX = (int)(sizeof(ga.g) / sizeof(ga.g[0]));
    for (int i = 0; i < MAX; ++i) {
        const int j = i < ga.count ? i : 0;
        g16.g[i] = ga.g[j];
        g16.h[i] = mirrors_of(j);
    }
    for (int i = 0; i <= MAX; ++i) g16.tile_start[i] = ga.tile_start[i];
    g16.count = ga.count; g16.xcd_map = ga.xcd_map;
}
// a bf16 mirror is usable as an operand when its rows are 4-byte aligned (AIR_GEMM_BF16_STORAGE=0: never)
static bool bf16_storage() {
    static const int use16 = getenv("AIR_GEMM_BF16_STORAGE") ? atoi(getenv("AIR_GEMM_BF16_STORAGE")) : 1;
    return use16 != 0;
}
static inline bool mirror_usable(const void *m16, int ld) { return m16 && ld % 2 == 0 && ((uintptr_t)m16 % 4 == 0); }

// 16x16 tiles of the problems outside skip_mask: the measure of a group's size that every tile rule below is stated in
static long group_tiles16(const AirGemmDesc *descs, int count, unsigned skip_mask) {
    long tiles16 = 0;
    for (int i = 0; i < count; ++i)
        if (!((skip_mask >> i) & 1u)) tiles16 += (long)air_cdiv(descs[i].M, 16) * air_cdiv(descs[i].N, 16);
    return tiles16;
}
// tile shape for the whole group: 16x16 tiles (more, shorter-lived workgroups) while the group is far from filling
// the chip, 32x32 tiles once it holds thousands of them (less operand re-read, fewer workgroup rounds)
static inline int latency_tile(long tiles16) { return air_gemm_latency_tile(tiles16); }
// long K on a handful of tiles (the BPTT products, 64x256x1024): 16 waves split K inside the workgroup, so every wave
// still needs only one or two memory round trips and no second (split-K epilogue) launch is paid
static bool group_long_k(const AirGemmDesc *descs, int count, long tiles16) {
    bool long_k = tiles16 <= 1024;
    for (int i = 0; i < count; ++i) long_k = long_k && air_gemm_long_k(descs[i].M, descs[i].N, descs[i].K);
    return long_k;
}
// one precision per launch: problem d against the launch's (bf), and a whole group against its first problem's
static int problem_precision(const AirGemmDesc &d, bool bf) {
    AIR_REQUIRE(d.precision == AIR_PREC_F32 || d.precision == AIR_PREC_BF16, AIR_E_UNSUPPORTED);
    AIR_REQUIRE((d.precision == AIR_PREC_BF16) == bf, AIR_E_UNSUPPORTED);
    return AIR_OK;
}
static int group_precision(const AirGemmDesc *descs, int count, bool *bf) {
    *bf = descs[0].precision == AIR_PREC_BF16;
    for (int i = 0; i < count; ++i)
        if (int st = problem_precision(descs[i], *bf)) return st;
    return AIR_OK;
}

// ---- the wide-tile (throughput) regime of a group of at most AIR_GEMM_GROUP_MAX problems ---------------------------------------
static long wide_min_tiles() { return air_gemm_wide_min_tiles(); }
// A group air_gemm_grouped is SURE to run on the 16-wave K-split body, whatever its layouts and alignment: group_long_k, and too few
// tiles for the wide-tile regime, which air_gemm_grouped tests first (a larger long-K group stays on the K split only where
// wide_group_eligible turns it down for its layout or alignment: the launches that fold into that body do not take those).
static bool group_on_long_k_body(const AirGemmDesc *descs, int count, long tiles16) {
    return tiles16 <= wide_min_tiles() && group_long_k(descs, count, tiles16);
}
// The full rule (air_gemm_grouped): the wide-tile kernels (every operand load 16 bytes per lane) when the whole group has one
// operand layout and every problem meets the alignment the interleaved loads need.  *min_k = the shortest K, *nt_short = a dX
// group (both operands k-contiguous) below the K from which the 16x64 tile pays.
static bool wide_group_eligible(const AirGemmDesc *descs, int count, long tiles16, bool bf, int *min_k_out, bool *nt_short_out) {
    static const long wide_tn_bf = getenv("AIR_GEMM_WIDE_TN_BF16") ? atol(getenv("AIR_GEMM_WIDE_TN_BF16")) : 48;
    static const long wide_tn_f32 = getenv("AIR_GEMM_WIDE_TN_F32") ? atol(getenv("AIR_GEMM_WIDE_TN_F32")) : 48;
    static const long wide_nt_k = getenv("AIR_GEMM_WIDE_NT_K") ? atol(getenv("AIR_GEMM_WIDE_NT_K")) : 512;
    bool ok = tiles16 > wide_min_tiles();
    const int ta = descs[0].ta ? 1 : 0, tb = descs[0].tb ? 1 : 0;
    long tiles64 = 0;
    int min_k = 1 << 30;
    for (int i = 0; i < count && ok; ++i) {
        const AirGemmDesc &d = descs[i];
        ok = ok && (d.ta ? 1 : 0) == ta && (d.tb ? 1 : 0) == tb && !(ta && tb) && !d.A2;
        // 16-byte operand loads need not be 16-byte aligned (any leading dimension of A; K of any length when A is
        // k-contiguous); an interleaved operand must hold whole groups of 4 rows / columns; B as the weights are laid out
        ok = ok && air_aligned16(d.B) && d.ldb % 4 == 0 && (!ta || d.K % 4 == 0) && (!tb || d.K % 4 == 0);
        ok = ok && d.M >= 4 && d.N >= 4 && d.K >= 4 && (!ta || d.M % 4 == 0) && (tb || d.N % 4 == 0);
        // (the unaligned / odd-K forms only where the launch is far into the throughput regime: around a thousand tiles
        //  the 16x16-tile kernel is the better one for them -- K = 50 leaves half of the 8 K-splitting waves idle)
        if (tiles16 <= 2048) ok = ok && air_aligned16(d.A) && d.lda % 4 == 0 && d.K % 4 == 0;
        tiles64 += (long)air_cdiv(d.M, 64) * air_cdiv(d.N, 64);
        if (d.K < min_k) min_k = d.K;
    }
    if (ok && ta) ok = tiles64 >= (bf ? wide_tn_bf : wide_tn_f32) && min_k >= 256;     // (K = rows: short at small batch)
    // dX products (both operands k-contiguous): the 16x64 tile pays from K = 512; below that a 32x64 tile is 10-20 % faster than
    // the 32x32-tile kernel with bf16 operands (L1 operand traffic) and no faster in fp32 (profiles/r02_j_kbench_gemm_*.txt)
    const bool nt_short = !ta && tb && min_k < wide_nt_k;
    if (ok && nt_short) ok = bf && tiles16 > 2048;
    *min_k_out = min_k; *nt_short_out = nt_short;
    return ok;
}
// What air_gemm_grouped_opt declines as "the wide-tile regime": a weight-gradient (all-TN) group of that size and depth, WITHOUT the
// alignment and tiles64 terms of the full rule -- deliberately weaker.  The folded launch is planned ahead of the buffers' addresses
// (engine_plan.py states the same three terms), and a weight-gradient group this large belongs to the deferred-gradient launch with
// its own fold whether or not every member meets the 16-byte rules, so such a group is declined here even where air_gemm_grouped
// itself would keep it on the tile kernels.
static bool wide_regime_weight_gradients(const AirGemmDesc *descs, int count, long tiles16) {
    int min_k = 1 << 30;
    bool all_tn = true;
    for (int i = 0; i < count; ++i) { all_tn = all_tn && descs[i].ta && !descs[i].tb; if (descs[i].K < min_k) min_k = descs[i].K; }
    return tiles16 > wide_min_tiles() && all_tn && min_k >= 256;
}

// ---- WHICH kernel air_gemm_grouped runs: one decision (gemm_grouped_form below), consumed by the launch code and returned by
// air_gemm_grouped_form.  Each *_form function validates the problems in the order the launch reports their errors. ---------------
static int validate_group(const AirGemmDesc *descs, int count) {
    GemmArgs scratch;
    for (int i = 0; i < count; ++i)
        if (int st = fill_gemm_args(scratch, descs[i])) return st;
    return AIR_OK;
}
// The workgroups problem i gets under a decided form: the ONE statement of the tile shapes -- the *_form functions add it up into
// f.workgroups, the launch code builds its workgroup ranges from it.
// (own8: the half tiles of gemm_grouped_longk_half_kernel, two bits per problem as there; 0 elsewhere)
static int form_workgroups_of(const AirGemmForm &f, int i, const AirGemmDesc &d, unsigned own8 = 0u) {
    switch (f.family) {
        case AIR_GEMM_FAM_BIG: case AIR_GEMM_FAM_BIG16:
            return ((f.small_mask >> i) & 1u) ? air_cdiv(d.M, 16) * air_cdiv(d.N, 16) : air_cdiv(d.M, 64) * air_cdiv(d.N, 64);
        case AIR_GEMM_FAM_WIDE: case AIR_GEMM_FAM_WIDE16:
            return air_cdiv(d.M, 16 * f.MT) * air_cdiv(d.N, 64);
        case AIR_GEMM_FAM_SHORTK:
            if ((f.sk_mask >> i) & 1u) return shortk_workgroups(d.M);
            [[fallthrough]];
        default:
            return air_cdiv(d.M, ((own8 >> (2 * i)) & 1u) ? 8 : f.tile) * air_cdiv(d.N, ((own8 >> (2 * i + 1)) & 1u) ? 8 : f.tile);
    }
}
static void form_sum_workgroups(AirGemmForm &f, const AirGemmDesc *descs, int count, unsigned own8 = 0u) {
    f.workgroups = 0;
    for (int i = 0; i < count; ++i) f.workgroups += form_workgroups_of(f, i, descs[i], own8);
}
// ---- half tiles for a launch the rule above puts on the 16-wave K split (family TILE, KW = 16) ------------------------------------
// Domain: fp32, every problem an NT product (both operands k-contiguous) without colsum whose epilogue is NONE or MUL_DELU -- the
// launch behind the BPTT.  AIR_GEMM_LONGK_TILE (air_common.h: air_tile_env) forces a shape for every problem of such a launch and is
// refused (AIR_E_UNSUPPORTED, nothing launched) by a 16-wave launch outside the domain; launches of the other forms do not read it.
// auto: 8x16 (GEMM_LONGK_TILE_AUTO) for a GROUP whose 16x16 tiling leaves at least half the CUs without a tile: what the A/B of the step
// adopted (profiles/half_tiles_ab.txt; 8x8 lost 5 us there).  *own8: two bits per problem (rows, columns halved), 0 = the 16x16 launch.
static constexpr bool GEMM_LONGK_TILE_AUTO = true;
static int longk_half_shapes(const AirGemmDesc *descs, int count, const AirGemmForm &f, long tiles16, unsigned *own8) {
    *own8 = 0u;
    if (f.family != AIR_GEMM_FAM_TILE || f.KW != 16) return AIR_OK;
    int shape = air_tile_env("AIR_GEMM_LONGK_TILE", "group");
    AIR_REQUIRE(shape != AIR_TILE_UNKNOWN, AIR_E_UNSUPPORTED);
    bool domain = !f.bf;
    for (int i = 0; i < count; ++i)
        domain = domain && !descs[i].ta && descs[i].tb && !descs[i].colsum &&
                 (descs[i].epilogue == AIR_EPI_NONE || descs[i].epilogue == AIR_EPI_MUL_DELU);
    AIR_REQUIRE(domain || shape == AIR_TILE_AUTO || shape == AIR_TILE_16x16, AIR_E_UNSUPPORTED);
    if (shape == AIR_TILE_AUTO) {
        shape = (GEMM_LONGK_TILE_AUTO && domain && count > 1 && 2 * tiles16 <= air_cu_count()) ? AIR_TILE_8x16 : AIR_TILE_16x16;
    }
    const unsigned per = shape == AIR_TILE_8x8 ? 3u : (shape == AIR_TILE_8x16 ? 1u : 0u);
    for (int i = 0; i < count; ++i) *own8 |= per << (2 * i);
    return AIR_OK;
}
// more than AIR_GEMM_GROUP_MAX problems: only the all-TN wide-tile form (the deferred weight gradients of a step)
static int big_tn_form(const AirGemmDesc *descs, int count, AirGemmForm &f) {
    AIR_REQUIRE(count <= AIR_GEMM_BIG_GROUP_MAX, AIR_E_SHAPE);
    const bool bf = descs[0].precision == AIR_PREC_BF16;
    int min_k = 1 << 30, n_wide = 0;
    GemmArgs scratch;
    for (int i = 0; i < count; ++i) {
        const AirGemmDesc &d = descs[i];
        if (int e = problem_precision(d, bf)) return e;
        AIR_REQUIRE(!d.A2, AIR_E_UNSUPPORTED);
        if (int e = fill_gemm_args(scratch, d)) return e;
        const bool wide = d.ta && !d.tb && air_aligned16(d.B) && d.ldb % 4 == 0 && d.K % 4 == 0 && d.M >= 4 && d.N >= 4 &&
                          d.M % 4 == 0 && d.N % 4 == 0;
        if (wide) {
            if (d.K < min_k) min_k = d.K;
            ++n_wide;
        } else f.small_mask |= 1u << i;
        // per-problem operand kinds: each problem reads the mirrors it has
        if (bf && bf16_storage() && mirror_usable(d.A16, d.lda)) f.a16_mask |= 1u << i;
        if (bf && bf16_storage() && mirror_usable(d.B16, d.ldb)) f.b16_mask |= 1u << i;
    }
    AIR_REQUIRE(n_wide > 0, AIR_E_UNSUPPORTED);            // this form exists for the weight gradients of a step
    // XCD-contiguous tiles: within each problem in fp32 (a map over the whole grid would hand every long-K problem -- they come
    // first -- to the first XCDs); over the whole grid with bf16 operands (launches of equal-K problems, L2-traffic bound)
    static const int big_xcd = getenv("AIR_GEMM_BIG_XCD") ? atoi(getenv("AIR_GEMM_BIG_XCD")) : 1;
    f.xcd_map = (big_xcd && min_k >= 1024) ? (bf ? 2 : 1) : 0;
    f.family = bf ? AIR_GEMM_FAM_BIG16 : AIR_GEMM_FAM_BIG;
    f.grouped = 1; f.MT = 4; f.KW = 8; f.bf = bf ? 1 : 0; f.ta = 1; f.tb = 0;
    f.threads = 512;
    form_sum_workgroups(f, descs, count);
    return AIR_OK;
}
static int launch_big_tn_group(const AirGemmDesc *descs, int count, const AirGemmForm &f, void *stream) {
    BigGroupArgs ga;
    int wt = 0;
    int st = fill_group(ga, descs, count, accept_any, [&](int i, const AirGemmDesc &d) { return form_workgroups_of(f, i, d); }, &wt);
    if (st) return st;
    ga.small_mask = f.small_mask;
    ga.xcd_map = f.xcd_map;
    hipStream_t stm = air_stream(stream);
    if (f.family == AIR_GEMM_FAM_BIG16) {
        BigGroupArgs16 g16;
        group_to16(g16, ga, [&](int j) {
            const AirGemmDesc &d = descs[j];
            return Gemm16Ptrs{((f.a16_mask >> j) & 1u) ? d.A16 : nullptr, ((f.b16_mask >> j) & 1u) ? d.B16 : nullptr, nullptr};
        });
        g16.small_mask = ga.small_mask;
        hipLaunchKernelGGL((gemm_big_group_wide16_tn_kernel<4, 8>), dim3(wt), dim3(512), 0, stm, g16);
    } else hipLaunchKernelGGL((gemm_big_group_wide_tn_kernel<4, 8, false>), dim3(wt), dim3(512), 0, stm, ga);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// a latency-regime group with short-K weight gradients among its problems: those on the streaming body, the rest on the 4-wave
// tile body (16x16 tiles, 32x32 once the REST holds more than 1536 of them), one launch
static unsigned shortk_mask(const AirGemmDesc *descs, int count) {
    unsigned m = 0;
    for (int i = 0; i < count; ++i) {
        if (descs[i].A2 || descs[i].C16 || descs[i].precision != AIR_PREC_F32) return 0;     // (the plain fp32 group only)
        if (shortk_eligible(descs[i])) m |= 1u << i;
    }
    return m;
}
static int launch_grouped_sk(const AirGemmDesc *descs, int count, const AirGemmForm &f, void *stream) {
    GroupArgs ga;
    int tiles = 0;
    int err = fill_group(ga, descs, count, accept_any, [&](int i, const AirGemmDesc &d) { return form_workgroups_of(f, i, d); }, &tiles);
    if (err) return err;
    ga.sk_mask = f.sk_mask;
    hipStream_t st = air_stream(stream);
    if (f.MT == 1) hipLaunchKernelGGL((gemm_grouped_sk_kernel<1, 1>), dim3(tiles), dim3(256), 0, st, ga);
    else hipLaunchKernelGGL((gemm_grouped_sk_kernel<2, 2>), dim3(tiles), dim3(256), 0, st, ga);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// air_gemm_grouped for the first product(s) of a train step whose input batch is drawn from an HBM-resident dataset: every problem's A
// operand lies inside the observation buffer g->obs [B, item_floats] (row 0 + a column offset, lda = item_floats) and is read from the
// dataset through the feeder's index instead; the problems of g->copy_mask write what they read into g->obs (together they must
// cover every column once); g->idx_out receives the indices.  16x16 tiles, 16 waves splitting K (the latency-regime form of these
// long-K products).  Returns AIR_E_UNSUPPORTED for anything else: the caller then plans air_batch_gather + air_gemm_grouped.
// The launch has ONE body, the 16-wave K split, so it takes only groups air_gemm_grouped itself runs on that body: group_on_long_k_body
// below.  (Until the kernel-level tests of the folded launches it asked for K >= 512 and at most 1024 tiles only.  Without
// K >= 8 min(M, N) a group such as M = 128, N = 256, K = 512 ran on 16 waves here and on the 4-wave body in the unfolded plan; and
// air_gemm_grouped tests the wide-tile regime BEFORE the long-K split, so an aligned NN group of wide_min_tiles() + 1 ... 1024 tiles
// such as 64 x 4096 x 2500 ran on 16 waves here and on gemm_wide_kernel there -- other partial sums, other bits, against the rule
// stated at shortk_eligible.  No shipped configuration has such a first layer; tests/test_fold_kernels.py keeps the shapes as declines.)
extern "C" int air_gemm_grouped_gather_fits(const AirGemmDesc *descs, int count, const AirBatchGather *g) {
    if (!descs || !g || count < 1 || count > AIR_GEMM_GROUP_MAX) return 0;
    if (!g->dataset || !g->obs || !g->seed_dev || !g->step_dev || g->n_items <= 0 || g->item_floats <= 0 || g->B <= 0) return 0;
    if (g->item_floats % 4 || !air_aligned16(g->dataset) || !air_aligned16(g->obs)) return 0;
    long tiles16 = 0;
    for (int i = 0; i < count; ++i) {
        const AirGemmDesc &d = descs[i];
        if (d.ta || d.A2 || d.C16 || d.precision != AIR_PREC_F32 || d.M != g->B || d.lda != g->item_floats) return 0;
        const long off = (const float *)d.A - (const float *)g->obs;
        if (off < 0 || off + d.K > g->item_floats || off % 4) return 0;
        tiles16 += (long)air_cdiv(d.M, 16) * air_cdiv(d.N, 16);
    }
    return group_on_long_k_body(descs, count, tiles16) ? 1 : 0;
}
extern "C" int air_gemm_grouped_gather(const AirGemmDesc *descs, int count, const AirBatchGather *g, void *stream) {
    AIR_REQUIRE(descs && g, AIR_E_NULL);
    AIR_REQUIRE(air_gemm_grouped_gather_fits(descs, count, g) == 1, AIR_E_UNSUPPORTED);
    GroupArgs ga;
    int tiles = 0;
    int err = fill_group(ga, descs, count, accept_any, [&](int i, const AirGemmDesc &d) {
        ga.g[i].vecA = 1;                                  // (dataset rows and column offsets are 16-byte aligned: checked above)
        return air_cdiv(d.M, 16) * air_cdiv(d.N, 16);
    }, &tiles);
    if (err) return err;
    const GatherArgs gt = {g->dataset, g->obs, g->obs, g->n_items, g->item_floats, g->shuffle ? 1 : 0, g->B, g->seed_dev, g->step_dev,
                           g->idx_out, g->copy_mask};
    hipLaunchKernelGGL(gemm_grouped_gather_kernel, dim3(tiles), dim3(1024), 0, air_stream(stream), ga, gt);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

static int gemm_grouped_form(const AirGemmDesc *descs, int count, AirGemmForm &f, unsigned *own8_out = nullptr) {
    memset(&f, 0, sizeof f);
    if (own8_out) *own8_out = 0u;
    if (count > AIR_GEMM_GROUP_MAX) return big_tn_form(descs, count, f);
    AIR_REQUIRE(count > 0 && count <= AIR_GEMM_GROUP_MAX, AIR_E_SHAPE);
    f.grouped = count > 1 ? 1 : 0;
    if (const unsigned skm = shortk_mask(descs, count)) {
        if (int err = validate_group(descs, count)) return err;
        f.family = AIR_GEMM_FAM_SHORTK; f.grouped = 1; f.sk_mask = skm;
        f.tile = latency_tile(group_tiles16(descs, count, skm));
        f.MT = f.NT = f.tile == 16 ? 1 : 2; f.KW = 4; f.threads = 256;
        form_sum_workgroups(f, descs, count);
        return AIR_OK;
    }
    const long tiles16 = group_tiles16(descs, count, 0u);
    const int T_ = latency_tile(tiles16);
    if (int err = validate_group(descs, count)) return err;
    const bool long_k = group_long_k(descs, count, tiles16);
    bool bf;
    if (int err = group_precision(descs, count, &bf)) return err;
    f.bf = bf ? 1 : 0;
    {   // throughput regime
        const int ta = descs[0].ta ? 1 : 0, tb = descs[0].tb ? 1 : 0;
        int min_k;
        bool nt_short;
        const bool ok = wide_group_eligible(descs, count, tiles16, bf, &min_k, &nt_short);
        if (ok && bf && ta) {   // per-problem operand kinds (mirrors) in one launch
            memset(&f, 0, sizeof f);
            return big_tn_form(descs, count, f);
        }
        if (ok) {
            f.family = bf ? AIR_GEMM_FAM_WIDE16 : AIR_GEMM_FAM_WIDE;
            f.ta = ta; f.tb = tb; f.nt_short = nt_short ? 1 : 0;
            f.MT = ta ? 4 : (nt_short ? 2 : 1); f.KW = 8; f.threads = 512;
            form_sum_workgroups(f, descs, count);
            // long-K weight-gradient groups (1.5 MB of operands per tile): measured +1.3 % on the batch-1024 step with bf16
            // operands, nothing in fp32 (MFMA issue bound), -1.5 % at batch 256 (K = 768)
            f.xcd_map = (ta && min_k >= 1024) ? 1 : 0;
            if (bf) {
                // the bf16 data path: operands from their bf16 mirrors where EVERY problem of the launch has one (4-byte
                // aligned rows), from the fp32 buffers otherwise; mirrors of C written by the epilogue
                bool a16 = bf16_storage(), b16 = bf16_storage();
                for (int i = 0; i < count; ++i) {
                    a16 = a16 && mirror_usable(descs[i].A16, descs[i].lda);
                    b16 = b16 && mirror_usable(descs[i].B16, descs[i].ldb);
                }
                f.a16_mask = a16 ? (1u << count) - 1u : 0u;
                f.b16_mask = b16 ? (1u << count) - 1u : 0u;
            }
            return AIR_OK;
        }
    }
    for (int i = 0; i < count; ++i) AIR_REQUIRE(!descs[i].A2 || count == 1, AIR_E_UNSUPPORTED);
    bool any_c16 = false;
    for (int i = 0; i < count; ++i) any_c16 = any_c16 || (descs[i].C16 != nullptr);
    f.tile = T_; f.long_k = long_k ? 1 : 0;
    f.MT = f.NT = (long_k || T_ == 16) ? 1 : 2; f.KW = long_k ? 16 : 4; f.threads = 64 * f.KW;
    if (any_c16) {
        // bf16 data path on small tiles: fp32 operand fetch, rounded in registers; the epilogue also writes the bf16 mirror of C
        AIR_REQUIRE(bf && !descs[0].A2, AIR_E_UNSUPPORTED);
        f.family = AIR_GEMM_FAM_C16;
    } else if (count == 1 && descs[0].A2) {
        // latency-regime consumer of a K-split producer; a long K (the first hidden layer >= 512 wide at a small batch) stays
        // on the 4-wave prologue kernel: correct for any K, the 16-wave K split has no prologue form
        AIR_REQUIRE(T_ == 16, AIR_E_UNSUPPORTED);
        f.family = AIR_GEMM_FAM_APRO; f.MT = f.NT = 1; f.KW = 4; f.threads = 256;
    } else f.family = AIR_GEMM_FAM_TILE;
    unsigned own8;
    if (int err = longk_half_shapes(descs, count, f, tiles16, &own8)) return err;
    if (own8) { f.grouped = 1; f.small_mask = (1u << count) - 1u; }        // half tiles: always the grouped kernel
    if (own8_out) *own8_out = own8;
    form_sum_workgroups(f, descs, count, own8);
    return AIR_OK;
}
extern "C" int air_gemm_grouped_form(const AirGemmDesc *descs, int count, AirGemmForm *out) {
    AIR_REQUIRE(descs && out, AIR_E_NULL);
    return gemm_grouped_form(descs, count, *out);
}

extern "C" int air_gemm_grouped(const AirGemmDesc *descs, int count, void *stream) {
    AIR_REQUIRE(descs, AIR_E_NULL);
    AirGemmForm f;
    unsigned own8 = 0u;
    if (int err = gemm_grouped_form(descs, count, f, &own8)) return err;
    if (f.family == AIR_GEMM_FAM_BIG || f.family == AIR_GEMM_FAM_BIG16) return launch_big_tn_group(descs, count, f, stream);
    if (f.family == AIR_GEMM_FAM_SHORTK) return launch_grouped_sk(descs, count, f, stream);
    GroupArgs ga;
    int tiles = 0;
    const bool wide = f.family == AIR_GEMM_FAM_WIDE || f.family == AIR_GEMM_FAM_WIDE16;
    int err = fill_group(ga, descs, count, accept_any, [&](int i, const AirGemmDesc &d) { return form_workgroups_of(f, i, d, own8); }, &tiles);
    if (err) return err;
    hipStream_t st = air_stream(stream);
    const bool bf = f.bf != 0;
    if (own8) {
        hipLaunchKernelGGL(gemm_grouped_longk_half_kernel, dim3(tiles), dim3(1024), 0, st, ga, own8);
        AIR_LAUNCH_CHECK();
        return AIR_OK;
    }
    if (wide) {
        const int wt = tiles;
        ga.xcd_map = f.xcd_map;
        if (bf) {
            const bool a16 = f.a16_mask != 0u, b16 = f.b16_mask != 0u;
            GroupArgs16 g16;
            group_to16(g16, ga, [&](int j) {
                return Gemm16Ptrs{a16 ? descs[j].A16 : nullptr, b16 ? descs[j].B16 : nullptr, descs[j].C16};
            });
#define AIR_WIDE16_LAUNCH2(MT_, TA_, TB_, A16_, B16_)                                                                              \
            do {                                                                                                           \
                if (!f.grouped) hipLaunchKernelGGL((gemm_wide16_kernel<MT_, 8, TA_, TB_, A16_, B16_>), dim3(wt), dim3(512), 0, st, g16.g[0], g16.h[0]); \
                else hipLaunchKernelGGL((gemm_grouped_wide16_kernel<MT_, 8, TA_, TB_, A16_, B16_>), dim3(wt), dim3(512), 0, st, g16);                   \
            } while (0)
#define AIR_WIDE16_LAUNCH(MT_, TA_, TB_)                                                                                   \
            do {                                                                                                           \
                if (a16 && b16) AIR_WIDE16_LAUNCH2(MT_, TA_, TB_, true, true);                                             \
                else if (a16) AIR_WIDE16_LAUNCH2(MT_, TA_, TB_, true, false);                                              \
                else if (b16) AIR_WIDE16_LAUNCH2(MT_, TA_, TB_, false, true);                                              \
                else AIR_WIDE16_LAUNCH2(MT_, TA_, TB_, false, false);                                                      \
            } while (0)
            // (<4, TN> is kept for the switch's sake only: gemm_grouped_form hands every bf16 TN group to the big-group launch)
            if (f.MT == 4) AIR_WIDE16_LAUNCH(4, true, false);
            else if (f.MT == 2) AIR_WIDE16_LAUNCH(2, false, true);
            else if (f.tb) AIR_WIDE16_LAUNCH(1, false, true);
            else AIR_WIDE16_LAUNCH(1, false, false);
#undef AIR_WIDE16_LAUNCH
#undef AIR_WIDE16_LAUNCH2
            AIR_LAUNCH_CHECK();
            return AIR_OK;
        }
#define AIR_WIDE_LAUNCH(MT_, TA_, TB_)                                                                                     \
        do {                                                                                                               \
            if (!f.grouped) hipLaunchKernelGGL((gemm_wide_kernel<MT_, 8, false, TA_, TB_>), dim3(wt), dim3(512), 0, st, ga.g[0]);         \
            else hipLaunchKernelGGL((gemm_grouped_wide_kernel<MT_, 8, false, TA_, TB_>), dim3(wt), dim3(512), 0, st, ga);                 \
        } while (0)
        // (<2, NT> is kept for the switch's sake only: wide_group_eligible admits the NT-short form with bf16 operands alone)
        if (f.MT == 4) AIR_WIDE_LAUNCH(4, true, false);
        else if (f.MT == 2) AIR_WIDE_LAUNCH(2, false, true);
        else if (f.tb) AIR_WIDE_LAUNCH(1, false, true);
        else AIR_WIDE_LAUNCH(1, false, false);
#undef AIR_WIDE_LAUNCH
        AIR_LAUNCH_CHECK();
        return AIR_OK;
    }
    // the tile families: <MT, NT, KW> = <1, 1, 16> (16 waves split K), <1, 1, 4> (16x16 tiles) or <2, 2, 4> (32x32 tiles; whole-tile
    // waves instead of a 4-way K split for short contractions were measured in round 3 and removed in round 4: 0.2131-0.2223
    // against 0.2077 ms at configs[1])
#define AIR_TILE_FORMS(LAUNCH_)                                                                                      \
    do {                                                                                                             \
        if (f.KW == 16) LAUNCH_(1, 1, 16, 1024);                                                                     \
        else if (f.MT == 1) LAUNCH_(1, 1, 4, 256);                                                                   \
        else LAUNCH_(2, 2, 4, 256);                                                                                  \
    } while (0)
#define AIR_GROUP_LAUNCH(MT_, NT_, KW_, NTH_)                                                                        \
    do {                                                                                                             \
        if (bf) hipLaunchKernelGGL((gemm_grouped_kernel<MT_, NT_, KW_, true>), dim3(tiles), dim3(NTH_), 0, st, ga);   \
        else hipLaunchKernelGGL((gemm_grouped_kernel<MT_, NT_, KW_, false>), dim3(tiles), dim3(NTH_), 0, st, ga);     \
    } while (0)
    // a lone problem goes through the single-GEMM kernel: its descriptor sits directly in the kernarg SGPRs, so the
    // tile_start lookup (one more dependent scalar-memory round trip before the first operand load) is skipped
#define AIR_SINGLE_LAUNCH(MT_, NT_, KW_, NTH_)                                                                       \
    do {                                                                                                             \
        if (bf) hipLaunchKernelGGL((gemm_f32_mfma_kernel<MT_, NT_, KW_, true>), dim3(tiles, 1), dim3(NTH_), 0, st, ga.g[0]);  \
        else hipLaunchKernelGGL((gemm_f32_mfma_kernel<MT_, NT_, KW_, false>), dim3(tiles, 1), dim3(NTH_), 0, st, ga.g[0]);    \
    } while (0)
    if (f.family == AIR_GEMM_FAM_C16) {
        C16Ptrs c16;
        for (int i = 0; i < AIR_GEMM_GROUP_MAX; ++i) c16.p[i] = i < count ? descs[i].C16 : nullptr;
#define AIR_C16_LAUNCH(MT_, NT_, KW_, NTH_)                                                                          \
        do {                                                                                                         \
            if (!f.grouped) hipLaunchKernelGGL((gemm_bf16_c16_kernel<MT_, NT_, KW_>), dim3(tiles, 1), dim3(NTH_), 0, st, ga.g[0], c16.p[0]);  \
            else hipLaunchKernelGGL((gemm_grouped_c16_kernel<MT_, NT_, KW_>), dim3(tiles), dim3(NTH_), 0, st, ga, c16);                     \
        } while (0)
        AIR_TILE_FORMS(AIR_C16_LAUNCH);
#undef AIR_C16_LAUNCH
    } else if (f.family == AIR_GEMM_FAM_APRO) {
        const AproArgs pro = {descs[0].A2, descs[0].a_bias, descs[0].a_out, descs[0].a_elu};
        if (bf) hipLaunchKernelGGL((gemm_f32_mfma_apro_kernel<1, 1, 4, true>), dim3(tiles, 1), dim3(256), 0, st, ga.g[0], pro);
        else hipLaunchKernelGGL((gemm_f32_mfma_apro_kernel<1, 1, 4, false>), dim3(tiles, 1), dim3(256), 0, st, ga.g[0], pro);
    } else if (!f.grouped) AIR_TILE_FORMS(AIR_SINGLE_LAUNCH);
    else AIR_TILE_FORMS(AIR_GROUP_LAUNCH);
#undef AIR_SINGLE_LAUNCH
#undef AIR_GROUP_LAUNCH
#undef AIR_TILE_FORMS
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// air_gemm_grouped with the backward of a Gaussian head (loc_mode 0) in the epilogue of problem `gb->problem` + NVIL / KL-share riders
// (include/air_hip.h).  Latency-regime tile kernels only.
extern "C" int air_gemm_grouped_gauss_bwd(const AirGemmDesc *descs, int count, const AirGaussBwdEpi *e, const float *imp_parts,
                                          int n_parts, float *imp_sum, const float *baseline, const float *logp, float *nvil_out,
                                          float *dlogp, float *dbaseline, int B, float *ema_dev, const float *kl_parts,
                                          int n_kl_parts, float *kl_row_out, int kl_rows, void *stream) {
    AIR_REQUIRE(descs && e, AIR_E_NULL);
    AIR_REQUIRE(count > 0 && count <= AIR_GEMM_GROUP_MAX && e->problem >= 0 && e->problem < count, AIR_E_SHAPE);
    AIR_REQUIRE(e->pre && e->eps && e->loc && e->scale && e->dpre && e->D > 0 && e->ld_pre >= 2 * e->D && e->ld_dpre >= 2 * e->D, AIR_E_NULL);
    AIR_REQUIRE(!imp_parts || (baseline && logp && nvil_out && B > 0 && n_parts > 0), AIR_E_NULL);
    AIR_REQUIRE(n_kl_parts >= 0 && (n_kl_parts == 0 || (kl_parts && kl_row_out && kl_rows > 0)), AIR_E_NULL);
    {
        const AirGemmDesc &d = descs[e->problem];          // the product that forms dsample[M, D]
        AIR_REQUIRE(d.N == e->D && d.beta == 0.f && d.epilogue == AIR_EPI_NONE && !d.colsum, AIR_E_UNSUPPORTED);
    }
    GroupArgs ga;
    const long tiles16 = group_tiles16(descs, count, 0u);
    AIR_REQUIRE(tiles16 <= 1000, AIR_E_UNSUPPORTED);         // (beyond: the 32x32 / wide-tile dispatch of air_gemm_grouped -- no fold there)
    int tiles = 0;
    const bool bf = descs[0].precision == AIR_PREC_BF16;
    int err = fill_group(ga, descs, count,
        [&](int, const AirGemmDesc &d) -> int {
            if (int e = problem_precision(d, bf)) return e;
            AIR_REQUIRE(!d.A2 && !d.C16, AIR_E_UNSUPPORTED);
            return AIR_OK;
        },
        [&](int, const AirGemmDesc &d) { return air_cdiv(d.M, 16) * air_cdiv(d.N, 16); }, &tiles);
    if (err) return err;
    const bool long_k = group_long_k(descs, count, tiles16);
    GaussEpi gb;
    gb.pre = e->pre; gb.eps = e->eps; gb.loc = e->loc; gb.scale = e->scale; gb.dkl_row = e->dkl_row; gb.dpre = e->dpre;
    gb.ld_pre = e->ld_pre; gb.ld_dpre = e->ld_dpre; gb.D = e->D; gb.raw_offset = e->raw_offset; gb.pl = e->p_loc; gb.ps = e->p_scale;
    gb.dkl_scale = e->dkl_scale; gb.guard = e->guard_eps; gb.mask = 1u << e->problem;
    const NvilArgs nv = {imp_parts, baseline, logp, nvil_out, dlogp, dbaseline, B, n_parts > 0 ? n_parts : 1, imp_sum, ema_dev};
    const KlParts kp = {kl_parts, kl_row_out, n_kl_parts};
    const int riders = (imp_parts ? 1 : 0) + (n_kl_parts > 0 ? 1 : 0);
    // (rider 0 is NVIL when there is one; the KL-share sum is the other -- or the only -- rider)
    hipStream_t st = air_stream(stream);
#define AIR_GB_LAUNCH(KW_, NTH_)                                                                                                   \
    do {                                                                                                                           \
        if (bf) hipLaunchKernelGGL((gemm_grouped_gb_kernel<1, 1, KW_, true>), dim3(tiles + riders), dim3(NTH_), 0, st, ga, gb, nv, kp, tiles, kl_rows);  \
        else hipLaunchKernelGGL((gemm_grouped_gb_kernel<1, 1, KW_, false>), dim3(tiles + riders), dim3(NTH_), 0, st, ga, gb, nv, kp, tiles, kl_rows);   \
    } while (0)
    if (long_k) AIR_GB_LAUNCH(16, 1024); else AIR_GB_LAUNCH(4, 256);
#undef AIR_GB_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// air_gemm_grouped with the optimiser folded in (include/air_hip.h): latency-regime tile kernels only (what the closing launch of
// the batch-64 train step runs on); a group the wide-tile dispatch would take is declined (AIR_E_UNSUPPORTED) -- the caller keeps
// the plain launch + air_step_epilogue there.
extern "C" int air_gemm_grouped_opt(const AirGemmDesc *descs, int count, const AirOptFold *o, void *stream) {
    AIR_REQUIRE(descs && o, AIR_E_NULL);
    AIR_REQUIRE(count > 0 && count <= AIR_GEMM_GROUP_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(o->p && o->g && o->ms && o->mg && o->mom && o->lr_dev, AIR_E_NULL);
    AIR_REQUIRE(o->n_ranges >= 0 && o->n_ranges <= AIR_OPT_MAX_RANGES && o->n_model % 4 == 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(o->p) && air_aligned16(o->g) && air_aligned16(o->ms) && air_aligned16(o->mg) && air_aligned16(o->mom), AIR_E_ALIGN);
    GroupArgs ga;
    // short-K weight gradients on the streaming body (their range = their workgroups).  A folded launch takes them when EVERY problem
    // is one (the engine's closing launch); a folded launch that mixes one with tile problems is declined -- the caller keeps the
    // unfolded launch + the closing update for it, so the product is the streaming body's in either plan
    const unsigned sk_mask = shortk_mask(descs, count);
    AIR_REQUIRE(sk_mask == 0 || sk_mask == (1u << count) - 1u, AIR_E_UNSUPPORTED);
    const long tiles16 = group_tiles16(descs, count, sk_mask);
    const int T_ = latency_tile(tiles16);
    int tiles = 0;
    const bool bf = descs[0].precision == AIR_PREC_BF16;
    int err = fill_group(ga, descs, count,
        [&](int, const AirGemmDesc &d) -> int {
            if (int e = problem_precision(d, bf)) return e;
            AIR_REQUIRE(!d.A2 && !d.C16, AIR_E_UNSUPPORTED);
            return AIR_OK;
        },
        [&](int i, const AirGemmDesc &d) -> int {
            if ((o->fold_mask >> i) & 1u) {
                // a folded problem: a plain weight gradient written into the flat gradient buffer (its parameter sits at the same offset)
                AIR_REQUIRE(d.beta == 0.f && d.epilogue == AIR_EPI_NONE, AIR_E_UNSUPPORTED);
                AIR_REQUIRE(d.C >= o->g && (!d.colsum || d.colsum >= o->g), AIR_E_SHAPE);
            }
            return ((sk_mask >> i) & 1u) ? shortk_workgroups(d.M) : air_cdiv(d.M, T_) * air_cdiv(d.N, T_);
        }, &tiles);
    if (err) return err;
    const bool long_k = sk_mask == 0 && group_long_k(descs, count, tiles16);
    // the wide-tile regime has its own kernels (and its own fold, air_gemm_grouped's deferred-gradient launch): not here
    AIR_REQUIRE(!wide_regime_weight_gradients(descs, count, tiles16), AIR_E_UNSUPPORTED);
    OptFold f;
    f.p = o->p; f.g0 = o->g; f.ms = o->ms; f.mg = o->mg; f.mom = o->mom; f.n_model = o->n_model; f.lr_dev = o->lr_dev;
    f.lr_mult_tail = o->lr_mult_tail; f.decay = o->decay; f.momentum = o->momentum; f.eps = o->eps; f.gscale = o->grad_scale;
    f.fold_mask = o->fold_mask & ((1u << count) - 1u);
    f.n_ranges = o->n_ranges; f.tiles = tiles;
    size_t nq = 0;
    for (int r = 0; r < AIR_OPT_MAX_RANGES; ++r) {
        f.lo[r] = r < o->n_ranges ? o->range_lo[r] : 0; f.hi[r] = r < o->n_ranges ? o->range_hi[r] : 0;
        AIR_REQUIRE(f.lo[r] <= f.hi[r] && f.lo[r] % 4 == 0 && f.hi[r] % 4 == 0, AIR_E_SHAPE);
        nq += (f.hi[r] - f.lo[r]) >> 2;
    }
    f.gstep = o->global_step_dev; f.rng_state = o->rng_state_dev; f.rng_inc = o->rng_increment;
    const int nth = long_k ? 1024 : 256;
    size_t extra = air_rider_blocks(nq, nth, 512);                          // about two float4 per rider thread
    if (extra < 1) extra = 1;                                               // (the counters live in rider workgroup 0)
    hipStream_t st = air_stream(stream);
#define AIR_GROUP_OPT_LAUNCH(MT_, NT_, KW_)                                                                                                   \
    do {                                                                                                                                      \
        if (bf) hipLaunchKernelGGL((gemm_grouped_opt_kernel<MT_, NT_, KW_, true>), dim3(tiles + (int)extra), dim3(nth), 0, st, ga, f);         \
        else hipLaunchKernelGGL((gemm_grouped_opt_kernel<MT_, NT_, KW_, false>), dim3(tiles + (int)extra), dim3(nth), 0, st, ga, f);           \
    } while (0)
    ga.sk_mask = sk_mask;
    if (sk_mask) hipLaunchKernelGGL(gemm_grouped_opt_sk_kernel, dim3(tiles + (int)extra), dim3(256), 0, st, ga, f);
    else if (long_k) AIR_GROUP_OPT_LAUNCH(1, 1, 16);
    else if (T_ == 16) AIR_GROUP_OPT_LAUNCH(1, 1, 4);
    else AIR_GROUP_OPT_LAUNCH(2, 2, 4);
#undef AIR_GROUP_OPT_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ---- linear layer wrappers (neural.py:56-60) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void mul_delu_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                       float *__restrict__ g, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float yy = y[i];
        g[i] = dy[i] * (yy > 0.f ? 1.f : yy + 1.f);
    }
}

extern "C" int air_linear_fwd(const float *x, const float *w, const float *b, float *y, int M, int K, int N, int act,
                              void *ws, size_t ws_bytes, void *stream) {
    AIR_REQUIRE(act == AIR_ACT_NONE || act == AIR_ACT_ELU, AIR_E_UNSUPPORTED);
    AIR_REQUIRE(act == AIR_ACT_NONE || b, AIR_E_NULL);
    const int epi = (act == AIR_ACT_ELU) ? AIR_EPI_BIAS_ELU : (b ? AIR_EPI_BIAS : AIR_EPI_NONE);
    return air_gemm(0, 0, M, N, K, x, K, w, N, y, N, b, epi, nullptr, 0, 0.f, nullptr, ws, ws_bytes, stream);
}

extern "C" int air_linear_bwd(const float *x, const float *w, const float *y, const float *dy, float *dx, float *dw,
                              float *db, float *gbuf, int M, int K, int N, int act, void *ws, size_t ws_bytes,
                              void *stream) {
    AIR_REQUIRE(x && w && dy && dw, AIR_E_NULL);
    AIR_REQUIRE(act == AIR_ACT_NONE || act == AIR_ACT_ELU, AIR_E_UNSUPPORTED);
    const float *g = dy;
    if (act == AIR_ACT_ELU) {
        AIR_REQUIRE(y && gbuf, AIR_E_NULL);
        const size_t n = (size_t)M * N;
        int blocks = (int)((n + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(mul_delu_kernel, dim3(blocks), dim3(256), 0, air_stream(stream), dy, y, gbuf, n);
        AIR_LAUNCH_CHECK();
        g = gbuf;
    }
    int st;
    if (dx) {   // dx[M,K] = g[M,N] . w[K,N]^T
        st = air_gemm(0, 1, M, K, N, g, N, w, N, dx, K, nullptr, AIR_EPI_NONE, nullptr, 0, 0.f, nullptr, ws, ws_bytes, stream);
        if (st) return st;
    }
    // dw[K,N] = x[M,K]^T . g[M,N]; db = colsum(g)
    st = air_gemm(1, 0, K, N, M, x, K, g, N, dw, N, nullptr, AIR_EPI_NONE, nullptr, 0, 0.f, db, ws, ws_bytes, stream);
    return st;
}
