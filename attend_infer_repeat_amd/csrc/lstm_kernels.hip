// The fused LSTM steps and the `what` head: GEMM-shaped kernels of their own (own extern "C" entries) that share only the operand
// loaders and MFMA helpers of gemm_device.h with the GEMM family (gemm_kernels.hip).
#include "air_common.h"
#include "prologue_device.h"
#include "optimizer_device.h"
#include "engine_device.h"
#include "nvil_device.h"
#include "gemm_device.h"

// ---- LSTM recurrence with the gate math fused into the GEMM (snt.LSTM, mnist_model.py:35 / cell.py:126-127) -----------
// The recurrence is the one truly sequential part of the step (T dependent products that cannot be batched over time),
// and at batch 64 each link of that chain costs a launch (~4.5 us) far more than its flops.  Fusing the gate
// non-linearities into the product halves the chain: forward T launches instead of 2T, backward T instead of 2T+1.
//
// One 16x16 accumulator tile per workgroup, KW waves interleave the 16-deep K chunks (as gemm_body<1,1,KW>); A is always
// k-contiguous, B is k-strided (forward: W_h[K=Hd, 4Hd]) or k-contiguous (backward: W_h read as [N=Hd, K=4Hd]).
// (MASK: lanes whose row / column is not ok issue NO load in the full chunks instead of a clamped one -- the half tiles of the BPTT link)
template <int KW, bool BF, bool B_KCONTIG, bool MASK = false>
__device__ __forceinline__ void tile16_kloop(f32x4 (&acc)[1][1], gcf gA, int lda, int rowA, bool okA, bool vecA, gcf gB,
                                             int ldb, int colB, bool okB, bool vecB, int K, int limA, int limB) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4;
    constexpr int U = 4;
    const int full_end = K >> 4;
    const int rowAc = okA ? rowA : limA - 1, colBc = okB ? colB : limB;
#pragma nounroll
    for (int c = wave; c < full_end; c += U * KW) {
        f32x4 fa[U][1], fb[U][1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cu = c + u * KW;
            if (cu < full_end) {
                const int k = (cu << 4) + 4 * lg;
                fa[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
                fb[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (!MASK || okA) fa[u][0] = ld_kcontig_full(gA, lda, rowAc, k, vecA);
                if (!MASK || okB) fb[u][0] = B_KCONTIG ? ld_kcontig_full(gB, ldb, colBc, k, vecB) : ld_kstrided_full(gB, ldb, colBc, k);
            } else {
                fa[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
                fb[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW >= full_end) break;
            mfma_chunk<1, 1, BF>(acc, fa[u], fb[u]);
        }
    }
    const int pc = K >> 4;
    if ((K & 15) && (pc % KW) == wave) {
        const int k = (pc << 4) + 4 * lg;
        f32x4 fa[1], fb[1];
        fa[0] = ld_kcontig(gA, lda, rowA, okA, k, K, vecA);
        fb[0] = B_KCONTIG ? ld_kcontig(gB, ldb, colB, okB, k, K, vecB) : ld_kstrided(gB, ldb, colB, okB, k, K);
        mfma_chunk<1, 1, BF>(acc, fa, fb);
    }
}

// Two independent contractions of one tile position with the loads of BOTH issued before the first MFMA (the first LSTM step with
// the folded input product: x . W_x and h0 . W_h): one memory round trip instead of two per group of U chunks.  Chunk c of segment s
// goes to the wave tile16_kloop gives it to, and each segment accumulates its chunks in tile16_kloop's order: same bits.
template <int KW, bool BF>
__device__ __forceinline__ void tile16_kloop2(f32x4 (&acc0)[1][1], f32x4 (&acc1)[1][1], gcf gA0, int lda0, bool vecA0, gcf gB0, int K0,
                                              gcf gA1, int lda1, bool vecA1, gcf gB1, int K1, int ldb, int rowA, bool okA, int colB,
                                              bool okB, int limA, int limB) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4;
    constexpr int U = 4;
    const int full0 = K0 >> 4, full1 = K1 >> 4;
    const int rowAc = okA ? rowA : limA - 1, colBc = okB ? colB : limB;
    const int fmax = full0 > full1 ? full0 : full1;
#pragma nounroll
    for (int c = wave; c < fmax; c += U * KW) {
        f32x4 fa0[U][1], fb0[U][1], fa1[U][1], fb1[U][1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cu = c + u * KW;
            const int k = (cu << 4) + 4 * lg;
            if (cu < full0) { fa0[u][0] = ld_kcontig_full(gA0, lda0, rowAc, k, vecA0); fb0[u][0] = ld_kstrided_full(gB0, ldb, colBc, k); }
            else { fa0[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; fb0[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
            if (cu < full1) { fa1[u][0] = ld_kcontig_full(gA1, lda1, rowAc, k, vecA1); fb1[u][0] = ld_kstrided_full(gB1, ldb, colBc, k); }
            else { fa1[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; fb1[u][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW < full0) mfma_chunk<1, 1, BF>(acc0, fa0[u], fb0[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW < full1) mfma_chunk<1, 1, BF>(acc1, fa1[u], fb1[u]);
        }
    }
    const int pc0 = K0 >> 4, pc1 = K1 >> 4;
    if ((K0 & 15) && (pc0 % KW) == wave) {
        const int k = (pc0 << 4) + 4 * lg;
        f32x4 fa[1], fb[1];
        fa[0] = ld_kcontig(gA0, lda0, rowA, okA, k, K0, vecA0);
        fb[0] = ld_kstrided(gB0, ldb, colB, okB, k, K0);
        mfma_chunk<1, 1, BF>(acc0, fa, fb);
    }
    if ((K1 & 15) && (pc1 % KW) == wave) {
        const int k = (pc1 << 4) + 4 * lg;
        f32x4 fa[1], fb[1];
        fa[0] = ld_kcontig(gA1, lda1, rowA, okA, k, K1, vecA1);
        fb[0] = ld_kstrided(gB1, ldb, colB, okB, k, K1);
        mfma_chunk<1, 1, BF>(acc1, fa, fb);
    }
}

struct LstmFwdArgs {
    const float *h_prev, *w_h, *gx, *c_prev;
    float *h, *c, *gate_act;
    int M, Hd, ldw, ldgx, vecA;
    int ldh, ldc;            // row strides of h_prev / c_prev: Hd, or 0 = one row broadcast over the batch (trainable h0, c0)
    int tiles;               // workgroups [tiles, gridDim.x) run the step prologue instead (first step of a train step)
    float fb;
};
// tile = 16 batch rows x 4 hidden units: its 16 accumulator columns are the i,j,f,o gates of those 4 units (column
// 4*gate + unit  <->  W_h column gate*Hd + unit), so the gate math of a unit never leaves the workgroup
template <bool BF>
__global__ __launch_bounds__(256) void lstm_fwd_fused_kernel(LstmFwdArgs g, PrologueArgs pro) {
    constexpr int KW = 4, LDT = 20;
    __shared__ float s_tile[KW][16 * LDT];
    if ((int)blockIdx.x >= g.tiles) {       // independent role: noise / prior / tiled initial state for the rest of the step
        step_prologue_body(pro, (int)blockIdx.x - g.tiles, (int)gridDim.x - g.tiles);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_u = (g.Hd + 3) >> 2;
    const int tm = blockIdx.x / tiles_u, tu = blockIdx.x - tm * tiles_u;
    const int m0 = tm * 16, u0 = tu * 4;
    const int ub = u0 + (li & 3);
    const bool okB = ub < g.Hd;
    const int colB = (li >> 2) * g.Hd + ub;
    const int rowA = m0 + li;
    const bool okA = rowA < g.M;
    // epilogue operands of thread (r, uu): fetched before the K loop so their round trip overlaps the operand loads
    const int er = threadIdx.x >> 2, eu = u0 + (threadIdx.x & 3), em = m0 + er;
    const bool e_ok = threadIdx.x < 64 && em < g.M && eu < g.Hd;
    float e_gx[4] = {0.f, 0.f, 0.f, 0.f}, e_c = 0.f;
    if (e_ok) {
        const gcf gx = (gcf)g.gx + (size_t)em * g.ldgx + eu;
#pragma unroll
        for (int q = 0; q < 4; ++q) e_gx[q] = gx[(size_t)q * g.Hd];
        e_c = ((gcf)g.c_prev)[(size_t)em * g.ldc + eu];
    }
    f32x4 acc[1][1];
    acc[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    tile16_kloop<KW, BF, false>(acc, (gcf)g.h_prev, g.ldh, rowA, okA, g.vecA != 0, (gcf)g.w_h, g.ldw, colB, okB, false, g.Hd,
                                g.M, (li >> 2) * g.Hd + g.Hd - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) s_tile[wave][(4 * lg + r) * LDT + li] = acc[0][0][r];
    __syncthreads();
    if (e_ok) {
        float pre[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int off = er * LDT + 4 * q + (threadIdx.x & 3);
            pre[q] = ((s_tile[0][off] + s_tile[1][off]) + (s_tile[2][off] + s_tile[3][off])) + e_gx[q];
        }
        const float gi = sigmoid_acc(pre[0]);
        const float gj = tanhf(pre[1]);
        const float gf = sigmoid_acc(pre[2] + g.fb);
        const float go = sigmoid_acc(pre[3]);
        const float cn = gf * e_c + gi * gj;
        const size_t e = (size_t)em * g.Hd + eu;
        ((gf_t)g.c)[e] = cn;
        ((gf_t)g.h)[e] = tanhf(cn) * go;
        const gf_t ar = (gf_t)g.gate_act + (size_t)em * 4 * g.Hd + eu;
        ar[0] = gi; ar[g.Hd] = gj; ar[2 * (size_t)g.Hd] = gf; ar[3 * (size_t)g.Hd] = go;
    }
}

// The FIRST step of the unroll with the hoisted input product folded in (round 5: one dependent launch fewer on the forward chain).
// gx = x . W_x + b does not depend on t (the image never changes, cell.py:121-125), so it used to be a launch of its own in front of
// the recurrence; but step 0's recurrent operand is the trainable initial state -- ONE row for the whole batch -- so its product
// h0 . W_h costs nothing to add here: the tile accumulates BOTH contractions (x[M,E] . W_x[E,4Hd] and h0[1,Hd] . W_h[Hd,4Hd]) into
// two accumulators, writes gx = (x . W_x) + b for the later steps and finishes step 0's gate math on gx + h0 . W_h -- the same
// sums in the same order as the two launches it replaces (bit-identical h_1, c_1, gate_act_0, gx).
struct LstmFirstArgs { const float *x, *w_x, *b; float *gx_out; int E, ldx, vecX; };
template <bool BF>
__global__ __launch_bounds__(256) void lstm_fwd_first_kernel(LstmFwdArgs g, LstmFirstArgs f, PrologueArgs pro) {
    constexpr int KW = 4, LDT = 20;
    __shared__ float s_x[KW][16 * LDT], s_h[KW][16 * LDT];
    if ((int)blockIdx.x >= g.tiles) {
        step_prologue_body(pro, (int)blockIdx.x - g.tiles, (int)gridDim.x - g.tiles);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_u = (g.Hd + 3) >> 2;
    const int tm = blockIdx.x / tiles_u, tu = blockIdx.x - tm * tiles_u;
    const int m0 = tm * 16, u0 = tu * 4;
    const int ub = u0 + (li & 3);
    const bool okB = ub < g.Hd;
    const int colB = (li >> 2) * g.Hd + ub;
    const int rowA = m0 + li;
    const bool okA = rowA < g.M;
    const int er = threadIdx.x >> 2, eu = u0 + (threadIdx.x & 3), em = m0 + er;
    const bool e_ok = threadIdx.x < 64 && em < g.M && eu < g.Hd;
    float e_b[4] = {0.f, 0.f, 0.f, 0.f}, e_c = 0.f;
    if (e_ok) {
#pragma unroll
        for (int q = 0; q < 4; ++q) e_b[q] = ((gcf)f.b)[(size_t)q * g.Hd + eu];
        e_c = ((gcf)g.c_prev)[(size_t)em * g.ldc + eu];
    }
    f32x4 ax[1][1], ah[1][1];
    ax[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    ah[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int limB = (li >> 2) * g.Hd + g.Hd - 1;
    tile16_kloop2<KW, BF>(ax, ah, (gcf)f.x, f.ldx, f.vecX != 0, (gcf)f.w_x, f.E, (gcf)g.h_prev, g.ldh, g.vecA != 0, (gcf)g.w_h, g.Hd,
                          g.ldw, rowA, okA, colB, okB, g.M, limB);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s_x[wave][(4 * lg + r) * LDT + li] = ax[0][0][r];
        s_h[wave][(4 * lg + r) * LDT + li] = ah[0][0][r];
    }
    __syncthreads();
    if (e_ok) {
        float pre[4];
        const gf_t gxo = (gf_t)f.gx_out + (size_t)em * g.ldgx + eu;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int off = er * LDT + 4 * q + (threadIdx.x & 3);
            const float gxv = ((s_x[0][off] + s_x[1][off]) + (s_x[2][off] + s_x[3][off])) + e_b[q];      // the BIAS epilogue of the gx product
            gxo[(size_t)q * g.Hd] = gxv;
            pre[q] = ((s_h[0][off] + s_h[1][off]) + (s_h[2][off] + s_h[3][off])) + gxv;
        }
        const float gi = sigmoid_acc(pre[0]);
        const float gj = tanhf(pre[1]);
        const float gf = sigmoid_acc(pre[2] + g.fb);
        const float go = sigmoid_acc(pre[3]);
        const float cn = gf * e_c + gi * gj;
        const size_t e = (size_t)em * g.Hd + eu;
        ((gf_t)g.c)[e] = cn;
        ((gf_t)g.h)[e] = tanhf(cn) * go;
        const gf_t ar = (gf_t)g.gate_act + (size_t)em * 4 * g.Hd + eu;
        ar[0] = gi; ar[g.Hd] = gj; ar[2 * (size_t)g.Hd] = gf; ar[3 * (size_t)g.Hd] = go;
    }
}

// ---- the `what` head in ONE launch (round 5): q = x . W + b (modules.py:20-21), what ~ N(loc, softplus(raw + offset)) with its KL
// terms (cell.py:154-156, model.py:174-186) and the latent columns of the baseline input (modules.py:131-139) -- three things the
// step used to spend two dependent launches on (the product, then air_what_sample_pack).  A tile is 16 rows x 8 LATENT DIMS: its 16
// accumulator columns are the loc pre-activations of those dims AND their raw scales (gathered W columns a and A + a, the trick of the
// fused LSTM step), so after the in-workgroup K reduction a thread holds both halves of its (row, dim) and samples right there.  The
// KL row sum spans the ceil(A / 8) tiles of a row: each tile writes its 8-dim share to kl_parts[tile][M] (summed in the tile by three
// lane exchanges) and a later launch of the step adds the shares in tile order (air_gauss_sample_bwd*: kl_parts / kl_row_out).
struct WhatHeadArgs {
    const float *x, *w, *b, *eps;
    float *q, *loc, *scale, *what, *kl_parts, *pack;
    const float *where, *presence, *s0, *s1;
    int M, K, A, ldx, vecX, T, B, S0, S1, tiles;
    float raw_offset, pl, ps, guard;
};
template <bool BF>
__global__ __launch_bounds__(256) void what_head_kernel(WhatHeadArgs g) {
    constexpr int KW = 4, LDT = 20;
    __shared__ float s_tile[KW][16 * LDT];
    const int width = g.T * g.A + g.T * 4 + g.T + g.S0 + g.S1;
    if ((int)blockIdx.x >= g.tiles) {       // independent role: the where / presence / state columns of the baseline input
        baseline_pack_body((int)blockIdx.x - g.tiles, (int)gridDim.x - g.tiles, nullptr, g.what, g.where, g.presence, g.s0, g.s1,
                           g.pack, g.T, g.B, 0, g.A, g.S0, g.S1, g.T * g.A);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_n = (g.A + 7) >> 3;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * 16, a0 = tn * 8;
    const int ab = a0 + (li & 7);
    const bool okB = ab < g.A;
    const int colB = (li >> 3) * g.A + ab;
    const int rowA = m0 + li;
    const bool okA = rowA < g.M;
    const int er = threadIdx.x >> 3, ed = threadIdx.x & 7, em = m0 + er, ea = a0 + ed;
    const bool e_ok = threadIdx.x < 128 && em < g.M && ea < g.A;
    float e_bl = 0.f, e_br = 0.f, e_eps = 0.f;
    if (e_ok) {
        e_bl = ((gcf)g.b)[ea]; e_br = ((gcf)g.b)[g.A + ea];
        e_eps = ((gcf)g.eps)[(size_t)em * g.A + ea];
    }
    f32x4 acc[1][1];
    acc[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    tile16_kloop<KW, BF, false>(acc, (gcf)g.x, g.ldx, rowA, okA, g.vecX != 0, (gcf)g.w, 2 * g.A, colB, okB, false, g.K, g.M, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) s_tile[wave][(4 * lg + r) * LDT + li] = acc[0][0][r];
    __syncthreads();
    if (threadIdx.x < 128) {
        float kl = 0.f;
        if (e_ok) {
            const int o0 = er * LDT + ed, o1 = o0 + 8;
            const float locp = ((s_tile[0][o0] + s_tile[1][o0]) + (s_tile[2][o0] + s_tile[3][o0])) + e_bl;   // the BIAS epilogue
            const float raw = ((s_tile[0][o1] + s_tile[1][o1]) + (s_tile[2][o1] + s_tile[3][o1])) + e_br;
            const gf_t qr = (gf_t)g.q + (size_t)em * 2 * g.A;
            qr[ea] = locp; qr[g.A + ea] = raw;
            const float s = guard_scale(softplus_acc(raw + g.raw_offset), g.guard);
            const float v = locp + s * e_eps;
            const size_t o = (size_t)em * g.A + ea;
            ((gf_t)g.loc)[o] = locp; ((gf_t)g.scale)[o] = s; ((gf_t)g.what)[o] = v;
            const int t = em / g.B, bb = em - t * g.B;
            ((gf_t)g.pack)[(size_t)bb * width + t * g.A + ea] = v;
            kl = normal_kl(locp, s, g.pl, g.ps);
        }
        kl += __shfl_xor(kl, 1, 64);
        kl += __shfl_xor(kl, 2, 64);
        kl += __shfl_xor(kl, 4, 64);
        if (ed == 0 && em < g.M) ((gf_t)g.kl_parts)[(size_t)tn * g.M + em] = kl;
    }
}
extern "C" int air_what_head_parts(int A) { return (A + 7) / 8; }
extern "C" int air_what_head_fwd(const float *x, int ldx, int K, const float *w, const float *b, const float *eps, float raw_offset,
                                 float p_loc, float p_scale, float *q, float *loc, float *scale, float *sample, float *kl_parts,
                                 int A, const float *where, const float *presence, const float *state0, const float *state1,
                                 float *pack_out, int T, int B, int S0, int S1, float guard_eps, int precision, void *stream) {
    AIR_REQUIRE(x && w && b && eps && q && loc && scale && sample && kl_parts && where && presence && pack_out, AIR_E_NULL);
    AIR_REQUIRE((S0 == 0 || state0) && (S1 == 0 || state1), AIR_E_NULL);
    AIR_REQUIRE(T > 0 && B > 0 && A > 0 && K > 0 && ldx >= K && S0 >= 0 && S1 >= 0, AIR_E_SHAPE);
    AIR_REQUIRE(precision == AIR_PREC_F32 || precision == AIR_PREC_BF16, AIR_E_UNSUPPORTED);
    WhatHeadArgs g;
    g.x = x; g.w = w; g.b = b; g.eps = eps; g.q = q; g.loc = loc; g.scale = scale; g.what = sample; g.kl_parts = kl_parts; g.pack = pack_out;
    g.where = where; g.presence = presence; g.s0 = state0; g.s1 = state1;
    g.M = T * B; g.K = K; g.A = A; g.ldx = ldx; g.vecX = ((ldx % 4) == 0 && air_aligned16(x)) ? 1 : 0;
    g.T = T; g.B = B; g.S0 = S0; g.S1 = S1;
    g.tiles = air_cdiv(g.M, 16) * air_cdiv(A, 8);
    g.raw_offset = raw_offset; g.pl = p_loc; g.ps = p_scale; g.guard = guard_eps;
    const size_t n_pack = (size_t)B * (T * 5 + S0 + S1);
    int pb = (int)((n_pack + PW_THREADS - 1) / PW_THREADS);
    if (pb > 256) pb = 256;
    if (pb < 1) pb = 1;
    if (precision == AIR_PREC_BF16) hipLaunchKernelGGL((what_head_kernel<true>), dim3(g.tiles + pb), dim3(256), 0, air_stream(stream), g);
    else hipLaunchKernelGGL((what_head_kernel<false>), dim3(g.tiles + pb), dim3(256), 0, air_stream(stream), g);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ---- throughput regime (more than 512 tiles of 16 x 16): the same fusion on the wide-tile scheme ---------------------------
// Workgroup tile = 16 batch rows x 64 hidden units x the 4 gates: SIXTEEN 16-wide MFMA tiles per wave, tile (q, c) = gate q,
// units u0 + 4 i + c (i = 0..15).  W_h[k, q*Hd + u] is k-strided; per k step a lane issues FOUR 16-byte loads (one per gate,
// along the contiguous unit dimension) and every loaded value feeds a different tile -- no dword loads, no permuted copy of
// w_gates.  8 waves split K (Hd = 256: two 16-deep chunks each, all loads of a wave in ONE round trip) and reduce through LDS in
// a fixed order; the epilogue thread of (row, unit) then holds all four gates: `gates` never exists, one launch per step instead
// of a product and a pointwise pass.
template <bool BF>
__global__ __launch_bounds__(512) void lstm_fwd_wide_kernel(LstmFwdArgs g, PrologueArgs pro) {
    constexpr int KW = 8, LDT = 256 + 4;
    __shared__ float s_tile[KW][16 * LDT];                  // local column = gate * 64 + unit
    if ((int)blockIdx.x >= g.tiles) {
        if (threadIdx.x < PW_THREADS) step_prologue_body(pro, (int)blockIdx.x - g.tiles, (int)gridDim.x - g.tiles);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_u = g.Hd >> 6;
    const int tm = blockIdx.x / tiles_u, tu = blockIdx.x - tm * tiles_u;
    const int m0 = tm * 16, u0 = tu * 64;
    const gcf gA = (gcf)g.h_prev, gW = (gcf)g.w_h;
    int rowA = m0 + li; if (rowA > g.M - 1) rowA = g.M - 1;
    const size_t offA = (size_t)rowA * g.ldh;
    const int colb = u0 + 4 * li;
    // epilogue operands of this thread's two (row, unit) pairs, requested before the K loop
    float e_gx[2][4], e_c[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = threadIdx.x + 512 * i, r = e >> 6, u = e & 63;
        int m = m0 + r; if (m > g.M - 1) m = g.M - 1;
        const gcf gx = (gcf)g.gx + (size_t)m * g.ldgx + u0 + u;
#pragma unroll
        for (int q = 0; q < 4; ++q) e_gx[i][q] = gx[(size_t)q * g.Hd];
        e_c[i] = ((gcf)g.c_prev)[(size_t)m * g.ldc + u0 + u];
    }
    f32x4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int U = 2;
    const int nchunks = g.Hd >> 4;
#pragma nounroll
    for (int c = wave; c < nchunks; c += U * KW) {
        f32x4 fa[U], fw[U][4][4];                           // fw[u][j][q] = W_h[k + j, q*Hd + colb .. colb+3]
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int cu = c + u * KW; if (cu > nchunks - 1) cu = nchunks - 1;
            const int k = (cu << 4) + 4 * lg;
            fa[u] = *(gcf4)(gA + offA + k);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) fw[u][j][q] = *(gcf4)(gW + (size_t)(k + j) * g.ldw + (size_t)q * g.Hd + colb);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW >= nchunks) break;
            if (BF) {
                const s16x4 ha = to_bf16x4(fa[u]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        const s16x4 hb = to_bf16x4((f32x4){fw[u][0][q][cc], fw[u][1][q][cc], fw[u][2][q][cc], fw[u][3][q][cc]});
                        acc[q * 4 + cc] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ha, hb, acc[q * 4 + cc], 0, 0, 0);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc)
                            acc[q * 4 + cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][j], fw[u][j][q][cc], acc[q * 4 + cc], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *(f32x4 *)&s_tile[wave][(4 * lg + r) * LDT + q * 64 + 4 * li] =
                (f32x4){acc[q * 4 + 0][r], acc[q * 4 + 1][r], acc[q * 4 + 2][r], acc[q * 4 + 3][r]};
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = threadIdx.x + 512 * i, r = e >> 6, u = e & 63;
        const int m = m0 + r;
        float pre[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int off = r * LDT + q * 64 + u;
            float v = 0.f;
#pragma unroll
            for (int w4 = 0; w4 < KW; w4 += 4)
                v += (s_tile[w4][off] + s_tile[w4 + 1][off]) + (s_tile[w4 + 2][off] + s_tile[w4 + 3][off]);
            pre[q] = v + e_gx[i][q];
        }
        if (m < g.M) {
            const float gi = sigmoid_acc(pre[0]);
            const float gj = tanhf(pre[1]);
            const float gf = sigmoid_acc(pre[2] + g.fb);
            const float go = sigmoid_acc(pre[3]);
            const float cn = gf * e_c[i] + gi * gj;
            const size_t eo = (size_t)m * g.Hd + u0 + u;
            ((gf_t)g.c)[eo] = cn;
            ((gf_t)g.h)[eo] = tanhf(cn) * go;
            const gf_t ar = (gf_t)g.gate_act + (size_t)m * 4 * g.Hd + u0 + u;
            ar[0] = gi; ar[g.Hd] = gj; ar[2 * (size_t)g.Hd] = gf; ar[3 * (size_t)g.Hd] = go;
        }
    }
}

struct LstmBwdArgs {
    const float *dgates_next, *w_h, *dh_a, *dh_b, *dc_in, *gate_act, *c_prev, *c, *dgx_in;
    float *dgates, *dc_prev, *dgx_out;
    int M, Hd, vecA, vecB;
};
// dh[m,u] = sum_k dgates_{t+1}[m,k] W_h[u,k]  (+ the direct dh terms of step t), then the pointwise backward of step t for
// that (m,u): dgates_t (4 values), dc_{t-1}, and the running sum over time of dgates (what x.W_x receives) -- all
// element-wise in (m,u), so the 16x16 output tile finishes everything it owns
// (opt: an optimiser slice on the workgroups past the tiles -- a separate kernel argument, untouched by the tile workgroups)
//
// R x C (16x16, 8x16, 8x8): the part of the MFMA tile a workgroup OWNS.  Few 16x16 tiles with a long K (batch 64: 64 tiles, K = 1024)
// leave most CUs without a tile while each tile's CU takes in (16 + 16) K floats; a half tile spreads the same product over two or
// four times the workgroups at (R + C) K floats each.  Lanes li >= R (>= C) issue NO operand load (tile16_kloop, MASK: their
// fragments are zero) and the accumulator rows / columns they feed are never read.  An owned element sees the K chunks, the order
// inside a chunk and the reduction over the waves of the 16x16 tile: the same bits.
template <int KW, bool BF, int R = 16, int C = 16>
__global__ __launch_bounds__(64 * KW) void lstm_bwd_fused_kernel(LstmBwdArgs g, RmspropSlice opt) {
    constexpr int LDT = 20;
    __shared__ float s_tile[KW][16 * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_n = (g.Hd + C - 1) / C;
    {
        const int tiles = ((g.M + R - 1) / R) * tiles_n;
        if ((int)blockIdx.x >= tiles) {
            rmsprop_slice_body(opt, (int)blockIdx.x - tiles, (int)gridDim.x - tiles);
            return;
        }
    }
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * R, n0 = tn * C;
    const int rowA = m0 + li, colB = n0 + li;
    const bool okA = li < R && rowA < g.M, okB = li < C && colB < g.Hd;
    const int K = 4 * g.Hd;
    const int er = threadIdx.x / C, ec = threadIdx.x & (C - 1), em = m0 + er, eu = n0 + ec;
    const bool e_ok = threadIdx.x < R * C && em < g.M && eu < g.Hd;
    float gi = 0.f, gj = 0.f, gff = 0.f, go = 0.f, cp = 0.f, cc = 0.f, dha = 0.f, dhb = 0.f, dci = 0.f, sx[4] = {0.f, 0.f, 0.f, 0.f};
    if (e_ok) {
        const size_t e = (size_t)em * g.Hd + eu;
        const gcf ar = (gcf)g.gate_act + (size_t)em * K + eu;
        gi = ar[0]; gj = ar[g.Hd]; gff = ar[2 * (size_t)g.Hd]; go = ar[3 * (size_t)g.Hd];
        cp = ((gcf)g.c_prev)[e];
        cc = ((gcf)g.c)[e];
        if (g.dh_a) dha = ((gcf)g.dh_a)[e];
        if (g.dh_b) dhb = ((gcf)g.dh_b)[e];
        if (g.dc_in) dci = ((gcf)g.dc_in)[e];
        if (g.dgx_in) {
            const gcf sr = (gcf)g.dgx_in + (size_t)em * K + eu;
#pragma unroll
            for (int q = 0; q < 4; ++q) sx[q] = sr[(size_t)q * g.Hd];
        }
    }
    f32x4 acc[1][1];
    acc[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    tile16_kloop<KW, BF, true, (R < 16 || C < 16)>(acc, (gcf)g.dgates_next, K, rowA, okA, g.vecA != 0, (gcf)g.w_h, K, colB, okB, g.vecB != 0, K,
                                                   g.M, g.Hd - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) s_tile[wave][(4 * lg + r) * LDT + li] = acc[0][0][r];
    __syncthreads();
    if (e_ok) {
        const int off = er * LDT + ec;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < KW; q += 4)
            v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
        // same order as the unfused pair: the product accumulates ONTO the direct dh term (beta = 1), then + dh_b
        const float dh = (v + dha) + dhb;
        const float tc = tanhf(cc);
        const float dct = dci + dh * go * (1.f - tc * tc);
        float d[4];
        d[0] = dct * gj * gi * (1.f - gi);
        d[1] = dct * gi * (1.f - gj * gj);
        d[2] = dct * cp * gff * (1.f - gff);
        d[3] = dh * tc * go * (1.f - go);
        const gf_t dr = (gf_t)g.dgates + (size_t)em * K + eu;
#pragma unroll
        for (int q = 0; q < 4; ++q) dr[(size_t)q * g.Hd] = d[q];
        ((gf_t)g.dc_prev)[(size_t)em * g.Hd + eu] = dct * gff;
        if (g.dgx_out) {
            const gf_t so = (gf_t)g.dgx_out + (size_t)em * K + eu;
#pragma unroll
            for (int q = 0; q < 4; ++q) so[(size_t)q * g.Hd] = sx[q] + d[q];
        }
    }
}

// The ENTRY of the BPTT and its first link in ONE launch (latency regime, round 5): the pointwise backward of the last step T-1
// has no product in front of it -- it was a launch of its own (air_lstm_pointwise_bwd) whose only consumer is the link of step
// T-2.  Here every workgroup of that link forms its A operand dgates_{T-1}[16 rows, 4Hd] ON THE FLY from the saved gate activations,
// cell states and the two direct dh terms of step T-1 (wave w owns the unit chunks w, w+16, ...: the four gates of a unit chunk are
// four 16-deep chunks of K, so ONE set of loads yields four A fragments), multiplies it with W_h^T and finishes step T-2's gate
// backward exactly as lstm_bwd_fused_kernel does; the (row, unit) pairs of the tile's epilogue re-form their own step T-1 values for
// dc_in and the running sum over time.  The first column of tiles stores dgates_{T-1} / dc_{T-2 <- T-1} for the weight gradients.
// One element function for both places: same bits wherever it is evaluated.
struct LstmEntryArgs {
    const float *gate_act1, *c_prev1, *c1, *dh_a1, *dh_b1;     // step T-1 (dh_a1 / dh_b1 may be NULL)
    float *dgates1, *dc_prev1;
};
__device__ __forceinline__ void lstm_pw_bwd_elem(float gi, float gj, float gf, float go, float cp, float c, float dha, float dhb,
                                                 float dci, float (&d)[4], float &dc_prev) {
#pragma clang fp contract(off)
    // tanh through one v_exp_f32 and one v_rcp_f32 (absolute error ~1e-7; exact limits +-1): every workgroup of a row tile repeats
    // this for its 16 x Hd operand elements, and libm's tanhf is two thirds of that work (AIR_LSTM_ENTRY_TANHF: libm's, for A/B builds)
#ifdef AIR_LSTM_ENTRY_TANHF
    const float tc = tanhf(c);
#else
    const float tc = 1.f - __fdividef(2.f, __expf(2.f * c) + 1.f);
#endif
    const float dhe = dha + dhb;
    const float dct = dci + dhe * go * (1.f - tc * tc);
    d[0] = dct * gj * gi * (1.f - gi);
    d[1] = dct * gi * (1.f - gj * gj);
    d[2] = dct * cp * gf * (1.f - gf);
    d[3] = dhe * tc * go * (1.f - go);
    dc_prev = dct * gf;
}
// R x C: the owned part of the MFMA tile, as in lstm_bwd_fused_kernel (lanes li >= R load nothing and form a zero operand row, lanes
// li >= C load no weights; the first column of tiles stores the entry's own outputs: still one store per row tile).
template <int R, int C>
__global__ __launch_bounds__(1024) void lstm_bwd_entry_kernel(LstmBwdArgs g, LstmEntryArgs en, RmspropSlice opt) {
    constexpr int KW = 16, LDT = 20;
    __shared__ float s_tile[KW][16 * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_n = g.Hd / C;
    {
        const int tiles = ((g.M + R - 1) / R) * tiles_n;
        if ((int)blockIdx.x >= tiles) {
            rmsprop_slice_body(opt, (int)blockIdx.x - tiles, (int)gridDim.x - tiles);
            return;
        }
    }
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * R, n0 = tn * C;
    const int rowA = m0 + li, colB = n0 + (li & (C - 1));       // Hd % 16 == 0: every column of the tile exists
    const bool okA = li < R && rowA < g.M, okB = li < C;
    const int rowAc = rowA < g.M ? rowA : g.M - 1;
    const int Hd = g.Hd, K = 4 * Hd;
    // ---- epilogue operands of thread (er, ec): step T-2's, and step T-1's for dc_in and the running sum
    const int er = threadIdx.x / C, ec = threadIdx.x & (C - 1), em = m0 + er, eu = n0 + ec;
    const bool e_ok = threadIdx.x < R * C && em < g.M;
    float gi = 0.f, gj = 0.f, gff = 0.f, go = 0.f, cp = 0.f, cc = 0.f, dha = 0.f, dhb = 0.f;
    float gi1 = 0.f, gj1 = 0.f, gf1 = 0.f, go1 = 0.f, cp1 = 0.f, cc1 = 0.f, dha1 = 0.f, dhb1 = 0.f;
    if (e_ok) {
        const size_t e = (size_t)em * Hd + eu;
        const gcf ar = (gcf)g.gate_act + (size_t)em * K + eu;
        gi = ar[0]; gj = ar[Hd]; gff = ar[2 * (size_t)Hd]; go = ar[3 * (size_t)Hd];
        cp = ((gcf)g.c_prev)[e];
        cc = ((gcf)g.c)[e];
        if (g.dh_a) dha = ((gcf)g.dh_a)[e];
        if (g.dh_b) dhb = ((gcf)g.dh_b)[e];
        const gcf a1 = (gcf)en.gate_act1 + (size_t)em * K + eu;
        gi1 = a1[0]; gj1 = a1[Hd]; gf1 = a1[2 * (size_t)Hd]; go1 = a1[3 * (size_t)Hd];
        cp1 = ((gcf)en.c_prev1)[e];
        cc1 = ((gcf)en.c1)[e];
        if (en.dh_a1) dha1 = ((gcf)en.dh_a1)[e];
        if (en.dh_b1) dhb1 = ((gcf)en.dh_b1)[e];
    }
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nuc = Hd >> 4;                                     // unit chunks (16 units each)
    const gcf gW = (gcf)g.w_h + (size_t)colB * K;
#pragma nounroll
    for (int uc = wave; uc < nuc; uc += KW) {
        const int u4 = (uc << 4) + 4 * lg;
        const size_t eo = (size_t)rowAc * Hd + u4, ao = (size_t)rowAc * K + u4;
        // all loads of the group first: 4 gate vectors, 2 cell states, 2 dh terms, 4 weight fragments
        f32x4 a_g[4], fb[4];
        const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 v_cp = zero4, v_c = zero4, v_da = zero4, v_db = zero4;
#pragma unroll
        for (int q = 0; q < 4; ++q) { a_g[q] = zero4; fb[q] = zero4; }
        if (R == 16 || okA) {                                    // (half tiles: lanes outside the owned rows / columns load nothing)
#pragma unroll
            for (int q = 0; q < 4; ++q) a_g[q] = *(gcf4)((gcf)en.gate_act1 + ao + (size_t)q * Hd);
            v_cp = *(gcf4)((gcf)en.c_prev1 + eo); v_c = *(gcf4)((gcf)en.c1 + eo);
            if (en.dh_a1) v_da = *(gcf4)((gcf)en.dh_a1 + eo);
            if (en.dh_b1) v_db = *(gcf4)((gcf)en.dh_b1 + eo);
        }
        if (C == 16 || okB) {
#pragma unroll
            for (int q = 0; q < 4; ++q) fb[q] = *(gcf4)(gW + (size_t)q * Hd + u4);
        }
        f32x4 fa[4], v_dcp;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            float d[4], dcp;
            lstm_pw_bwd_elem(a_g[0][x], a_g[1][x], a_g[2][x], a_g[3][x], v_cp[x], v_c[x], v_da[x], v_db[x], 0.f, d, dcp);
            fa[0][x] = d[0]; fa[1][x] = d[1]; fa[2][x] = d[2]; fa[3][x] = d[3];
            v_dcp[x] = dcp;
        }
        if (tn == 0 && okA) {                                    // the entry's own outputs, once per row tile
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4 *)(en.dgates1 + ao + (size_t)q * Hd) = fa[q];
            *(f32x4 *)(en.dc_prev1 + eo) = v_dcp;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[q][j], fb[q][j], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s_tile[wave][(4 * lg + r) * LDT + li] = acc[r];
    __syncthreads();
    if (e_ok) {
        const int off = er * LDT + ec;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < KW; q += 4)
            v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
        float d1[4], dci;
        lstm_pw_bwd_elem(gi1, gj1, gf1, go1, cp1, cc1, dha1, dhb1, 0.f, d1, dci);     // step T-1 at this (row, unit)
        float d[4], dcp;
        lstm_pw_bwd_elem(gi, gj, gff, go, cp, cc, v + dha, dhb, dci, d, dcp);          // dh = (product + dh_a) + dh_b, as the link
        const gf_t dr = (gf_t)g.dgates + (size_t)em * K + eu;
#pragma unroll
        for (int q = 0; q < 4; ++q) dr[(size_t)q * Hd] = d[q];
        ((gf_t)g.dc_prev)[(size_t)em * Hd + eu] = dcp;
        if (g.dgx_out) {
            const gf_t so = (gf_t)g.dgx_out + (size_t)em * K + eu;
#pragma unroll
            for (int q = 0; q < 4; ++q) so[(size_t)q * Hd] = d1[q] + d[q];
        }
    }
}

// One BPTT link in the throughput regime: dh = dgates_{t+1}[M, 4Hd] . W_h[Hd, 4Hd]^T on the wide-tile scheme (both operands
// k-contiguous: 16 rows x 64 units per workgroup, 8 waves split the 4Hd-deep contraction), then -- exactly as
// lstm_bwd_fused_kernel -- the pointwise backward of step t for the (row, unit) pairs the tile owns.
template <bool BF>
__global__ __launch_bounds__(512) void lstm_bwd_wide_kernel(LstmBwdArgs g, RmspropSlice opt) {
    constexpr int KW = 8, NT = 4, LDT = 64 + 4;
    __shared__ float s_tile[KW][16 * LDT];
    const int tiles_n = g.Hd >> 6;
    {
        const int tiles = ((g.M + 15) >> 4) * tiles_n;
        if ((int)blockIdx.x >= tiles) {
            rmsprop_slice_body(opt, (int)blockIdx.x - tiles, (int)gridDim.x - tiles);
            return;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * 16, n0 = tn * 64;
    const int K = 4 * g.Hd;
    const gcf gA = (gcf)g.dgates_next, gB = (gcf)g.w_h;
    int rowA = m0 + li; if (rowA > g.M - 1) rowA = g.M - 1;
    const size_t offA = (size_t)rowA * K;
    size_t offB[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) offB[b] = (size_t)(n0 + 16 * b + li) * K;
    // epilogue operands of this thread's two (row, unit) pairs
    float gi[2], gj[2], gff[2], go[2], cp[2], cc[2], dha[2], dhb[2], dci[2], sx[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e_ = threadIdx.x + 512 * i, r = e_ >> 6, u = n0 + (e_ & 63);
        int m = m0 + r; if (m > g.M - 1) m = g.M - 1;
        const size_t e = (size_t)m * g.Hd + u;
        const gcf ar = (gcf)g.gate_act + (size_t)m * K + u;
        gi[i] = ar[0]; gj[i] = ar[g.Hd]; gff[i] = ar[2 * (size_t)g.Hd]; go[i] = ar[3 * (size_t)g.Hd];
        cp[i] = ((gcf)g.c_prev)[e];
        cc[i] = ((gcf)g.c)[e];
        dha[i] = g.dh_a ? ((gcf)g.dh_a)[e] : 0.f;
        dhb[i] = g.dh_b ? ((gcf)g.dh_b)[e] : 0.f;
        dci[i] = g.dc_in ? ((gcf)g.dc_in)[e] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) sx[i][q] = g.dgx_in ? ((gcf)g.dgx_in)[(size_t)m * K + u + (size_t)q * g.Hd] : 0.f;
    }
    f32x4 acc[1][NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[0][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    const int nchunks = K >> 4;
#pragma nounroll
    for (int c = wave; c < nchunks; c += U * KW) {
        f32x4 fa[U][1], fb[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int cu = c + u * KW; if (cu > nchunks - 1) cu = nchunks - 1;
            const int k = (cu << 4) + 4 * lg;
            fa[u][0] = *(gcf4)(gA + offA + k);
#pragma unroll
            for (int b = 0; b < NT; ++b) fb[u][b] = *(gcf4)(gB + offB[b] + k);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW >= nchunks) break;
            mfma_chunk<1, NT, BF>(acc, fa[u], fb[u]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int b = 0; b < NT; ++b) s_tile[wave][(4 * lg + r) * LDT + 16 * b + li] = acc[0][b][r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e_ = threadIdx.x + 512 * i, r = e_ >> 6, uc = e_ & 63, u = n0 + uc, m = m0 + r;
        const int off = r * LDT + uc;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < KW; q += 4) v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
        if (m >= g.M) continue;
        const float dh = (v + dha[i]) + dhb[i];                // same order as the unfused pair (beta = 1 accumulate, then + dh_b)
        const float tc = tanhf(cc[i]);
        const float dct = dci[i] + dh * go[i] * (1.f - tc * tc);
        float d[4];
        d[0] = dct * gj[i] * gi[i] * (1.f - gi[i]);
        d[1] = dct * gi[i] * (1.f - gj[i] * gj[i]);
        d[2] = dct * cp[i] * gff[i] * (1.f - gff[i]);
        d[3] = dh * tc * go[i] * (1.f - go[i]);
        const gf_t dr = (gf_t)g.dgates + (size_t)m * K + u;
#pragma unroll
        for (int q = 0; q < 4; ++q) dr[(size_t)q * g.Hd] = d[q];
        ((gf_t)g.dc_prev)[(size_t)m * g.Hd + u] = dct * gff[i];
        if (g.dgx_out) {
            const gf_t so = (gf_t)g.dgx_out + (size_t)m * K + u;
#pragma unroll
            for (int q = 0; q < 4; ++q) so[(size_t)q * g.Hd] = sx[i][q] + d[q];
        }
    }
}

// ---- the LSTM recurrence on the bf16 data path (throughput regime) -----------------------------------------------------------
// lstm_fwd_wide_kernel / lstm_bwd_wide_kernel with the operands in memory as bf16: W_h from the bf16 shadow of the parameters
// (half the bytes of the larger operand), h_prev / dgates_{t+1} from their mirrors where one exists (the previous step's launch
// wrote it; the first step reads the fp32 tiled initial state), products on v_mfma_f32_16x16x32_bf16, and the epilogue writes
// the mirrors of h / dgates / running dgx next to the fp32 values.  Same tiles, same fixed-order K split over 8 waves.
struct Lstm16 { const void *w16, *a16; void *out16, *out16_b; };
__global__ __launch_bounds__(512) void lstm_fwd_wide16_kernel(LstmFwdArgs g, Lstm16 x) {
    constexpr int KW = 8, LDT = 256 + 4;
    __shared__ float s_tile[KW][16 * LDT];                  // local column = gate * 64 + unit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tiles_u = g.Hd >> 6;
    const int tm = blockIdx.x / tiles_u, tu = blockIdx.x - tm * tiles_u;
    const int m0 = tm * 16, u0 = tu * 64;
    const gcf gA = (gcf)g.h_prev;
    const gch hA = (gch)x.a16, hW = (gch)x.w16;
    int rowA = m0 + li; if (rowA > g.M - 1) rowA = g.M - 1;
    const size_t offA = (size_t)rowA * g.ldh;
    const int colb = u0 + 4 * li;
    float e_gx[2][4], e_c[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = threadIdx.x + 512 * i, r = e >> 6, u = e & 63;
        int m = m0 + r; if (m > g.M - 1) m = g.M - 1;
        const gcf gx = (gcf)g.gx + (size_t)m * g.ldgx + u0 + u;
#pragma unroll
        for (int q = 0; q < 4; ++q) e_gx[i][q] = gx[(size_t)q * g.Hd];
        e_c[i] = ((gcf)g.c_prev)[(size_t)m * g.ldc + u0 + u];
    }
    f32x4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nchunks = g.Hd >> 5;                          // 32-deep chunks
#pragma nounroll
    for (int c = wave; c < nchunks; c += KW) {
        const int k = (c << 5) + 8 * lg;
        u32x4 fa;
        if (hA) fa = *(gcu4)(hA + offA + k);
        else fa = pk8(*(gcf4)(gA + offA + k), *(gcf4)(gA + offA + k + 4));
        u32x2 w[4][8];                                      // w[q][j] = W_h16[k + j, q*Hd + colb .. colb+3]
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q][j] = *(gcu2)(hW + (size_t)(k + j) * g.ldw + (size_t)q * g.Hd + colb);
        const bf16x8 ha = __builtin_bit_cast(bf16x8, fa);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[q * 4 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, __builtin_bit_cast(bf16x8, tr16<0>(w[q])), acc[q * 4 + 0], 0, 0, 0);
            acc[q * 4 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, __builtin_bit_cast(bf16x8, tr16<1>(w[q])), acc[q * 4 + 1], 0, 0, 0);
            acc[q * 4 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, __builtin_bit_cast(bf16x8, tr16<2>(w[q])), acc[q * 4 + 2], 0, 0, 0);
            acc[q * 4 + 3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, __builtin_bit_cast(bf16x8, tr16<3>(w[q])), acc[q * 4 + 3], 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *(f32x4 *)&s_tile[wave][(4 * lg + r) * LDT + q * 64 + 4 * li] =
                (f32x4){acc[q * 4 + 0][r], acc[q * 4 + 1][r], acc[q * 4 + 2][r], acc[q * 4 + 3][r]};
    __syncthreads();
    const gh_t h16 = (gh_t)x.out16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = threadIdx.x + 512 * i, r = e >> 6, u = e & 63;
        const int m = m0 + r;
        float pre[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int off = r * LDT + q * 64 + u;
            float v = 0.f;
#pragma unroll
            for (int w4 = 0; w4 < KW; w4 += 4)
                v += (s_tile[w4][off] + s_tile[w4 + 1][off]) + (s_tile[w4 + 2][off] + s_tile[w4 + 3][off]);
            pre[q] = v + e_gx[i][q];
        }
        if (m < g.M) {
            const float gi = sigmoid_acc(pre[0]);
            const float gj = tanhf(pre[1]);
            const float gf = sigmoid_acc(pre[2] + g.fb);
            const float go = sigmoid_acc(pre[3]);
            const float cn = gf * e_c[i] + gi * gj;
            const size_t eo = (size_t)m * g.Hd + u0 + u;
            const float hn = tanhf(cn) * go;
            ((gf_t)g.c)[eo] = cn;
            ((gf_t)g.h)[eo] = hn;
            if (h16) h16[eo] = bf16_bits(hn);
            const gf_t ar = (gf_t)g.gate_act + (size_t)m * 4 * g.Hd + u0 + u;
            ar[0] = gi; ar[g.Hd] = gj; ar[2 * (size_t)g.Hd] = gf; ar[3 * (size_t)g.Hd] = go;
        }
    }
}

__global__ __launch_bounds__(512) void lstm_bwd_wide16_kernel(LstmBwdArgs g, Lstm16 x) {
    constexpr int KW = 8, NT = 4, LDT = 64 + 4;
    __shared__ float s_tile[KW][16 * LDT];
    const int tiles_n = g.Hd >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * 16, n0 = tn * 64;
    const int K = 4 * g.Hd;
    const gcf gA = (gcf)g.dgates_next;
    const gch hA = (gch)x.a16, hB = (gch)x.w16;
    int rowA = m0 + li; if (rowA > g.M - 1) rowA = g.M - 1;
    const size_t offA = (size_t)rowA * K;
    size_t offB[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) offB[b] = (size_t)(n0 + 16 * b + li) * K;
    float gi[2], gj[2], gff[2], go[2], cp[2], cc[2], dha[2], dhb[2], dci[2], sx[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e_ = threadIdx.x + 512 * i, r = e_ >> 6, u = n0 + (e_ & 63);
        int m = m0 + r; if (m > g.M - 1) m = g.M - 1;
        const size_t e = (size_t)m * g.Hd + u;
        const gcf ar = (gcf)g.gate_act + (size_t)m * K + u;
        gi[i] = ar[0]; gj[i] = ar[g.Hd]; gff[i] = ar[2 * (size_t)g.Hd]; go[i] = ar[3 * (size_t)g.Hd];
        cp[i] = ((gcf)g.c_prev)[e];
        cc[i] = ((gcf)g.c)[e];
        dha[i] = g.dh_a ? ((gcf)g.dh_a)[e] : 0.f;
        dhb[i] = g.dh_b ? ((gcf)g.dh_b)[e] : 0.f;
        dci[i] = g.dc_in ? ((gcf)g.dc_in)[e] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) sx[i][q] = g.dgx_in ? ((gcf)g.dgx_in)[(size_t)m * K + u + (size_t)q * g.Hd] : 0.f;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    const int nchunks = K >> 5;
#pragma nounroll
    for (int c = wave; c < nchunks; c += U * KW) {
        u32x4 fa[U], fb[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int cu = c + u * KW; if (cu > nchunks - 1) cu = nchunks - 1;
            const int k = (cu << 5) + 8 * lg;
            if (hA) fa[u] = *(gcu4)(hA + offA + k);
            else fa[u] = pk8(*(gcf4)(gA + offA + k), *(gcf4)(gA + offA + k + 4));
#pragma unroll
            for (int b = 0; b < NT; ++b) fb[u][b] = *(gcu4)(hB + offB[b] + k);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KW >= nchunks) break;
#pragma unroll
            for (int b = 0; b < NT; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[u]), __builtin_bit_cast(bf16x8, fb[u][b]),
                                                                acc[b], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int b = 0; b < NT; ++b) s_tile[wave][(4 * lg + r) * LDT + 16 * b + li] = acc[b][r];
    __syncthreads();
    const gh_t d16 = (gh_t)x.out16, s16 = (gh_t)x.out16_b;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e_ = threadIdx.x + 512 * i, r = e_ >> 6, uc = e_ & 63, u = n0 + uc, m = m0 + r;
        const int off = r * LDT + uc;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < KW; q += 4) v += (s_tile[q][off] + s_tile[q + 1][off]) + (s_tile[q + 2][off] + s_tile[q + 3][off]);
        if (m >= g.M) continue;
        const float dh = (v + dha[i]) + dhb[i];
        const float tc = tanhf(cc[i]);
        const float dct = dci[i] + dh * go[i] * (1.f - tc * tc);
        float d[4];
        d[0] = dct * gj[i] * gi[i] * (1.f - gi[i]);
        d[1] = dct * gi[i] * (1.f - gj[i] * gj[i]);
        d[2] = dct * cp[i] * gff[i] * (1.f - gff[i]);
        d[3] = dh * tc * go[i] * (1.f - go[i]);
        const gf_t dr = (gf_t)g.dgates + (size_t)m * K + u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            dr[(size_t)q * g.Hd] = d[q];
            if (d16) d16[(size_t)m * K + u + (size_t)q * g.Hd] = bf16_bits(d[q]);
        }
        ((gf_t)g.dc_prev)[(size_t)m * g.Hd + u] = dct * gff[i];
        if (g.dgx_out) {
            const gf_t so = (gf_t)g.dgx_out + (size_t)m * K + u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float sv = sx[i][q] + d[q];
                so[(size_t)q * g.Hd] = sv;
                if (s16) s16[(size_t)m * K + u + (size_t)q * g.Hd] = bf16_bits(sv);
            }
        }
    }
}

extern "C" int air_lstm_step_fwd_bf16(const float *h_prev, const void *h_prev_bf16, const float *c_prev, const void *w_h_bf16,
                                      int ldw, const float *gx, int ldgx, float *h, void *h_bf16, float *c, float *gate_act,
                                      int M, int Hd, float forget_bias, void *stream) {
    AIR_REQUIRE(h_prev && c_prev && w_h_bf16 && gx && h && c && gate_act, AIR_E_NULL);
    AIR_REQUIRE(M > 0 && Hd > 0 && Hd % 64 == 0 && ldw >= 4 * Hd && ldw % 4 == 0 && ldgx >= 4 * Hd, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(h_prev) && ((uintptr_t)w_h_bf16 % 8 == 0) && (!h_prev_bf16 || (uintptr_t)h_prev_bf16 % 16 == 0), AIR_E_ALIGN);
    LstmFwdArgs g;
    g.h_prev = h_prev; g.w_h = nullptr; g.gx = gx; g.c_prev = c_prev; g.h = h; g.c = c; g.gate_act = gate_act;
    g.M = M; g.Hd = Hd; g.ldw = ldw; g.ldgx = ldgx; g.vecA = 1; g.ldh = Hd; g.ldc = Hd; g.fb = forget_bias;
    g.tiles = air_cdiv(M, 16) * (Hd / 64);
    const Lstm16 x = {w_h_bf16, h_prev_bf16, h_bf16, nullptr};
    hipLaunchKernelGGL(lstm_fwd_wide16_kernel, dim3(g.tiles), dim3(512), 0, air_stream(stream), g, x);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
extern "C" int air_lstm_step_bwd_bf16(const float *dgates_next, const void *dgates_next_bf16, const void *w_h_bf16,
                                      const float *dh_a, const float *dh_b, const float *dc_in, const float *gate_act,
                                      const float *c_prev, const float *c, const float *dgx_in, float *dgates,
                                      void *dgates_bf16, float *dc_prev, float *dgx_out, void *dgx_bf16, int M, int Hd,
                                      void *stream) {
    AIR_REQUIRE(dgates_next && w_h_bf16 && gate_act && c_prev && c && dgates && dc_prev, AIR_E_NULL);
    AIR_REQUIRE(M > 0 && Hd > 0 && Hd % 64 == 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(dgates_next) && ((uintptr_t)w_h_bf16 % 16 == 0) &&
                    (!dgates_next_bf16 || (uintptr_t)dgates_next_bf16 % 16 == 0), AIR_E_ALIGN);
    LstmBwdArgs g;
    g.dgates_next = dgates_next; g.w_h = nullptr; g.dh_a = dh_a; g.dh_b = dh_b; g.dc_in = dc_in; g.gate_act = gate_act;
    g.c_prev = c_prev; g.c = c; g.dgx_in = dgx_in; g.dgates = dgates; g.dc_prev = dc_prev; g.dgx_out = dgx_out;
    g.M = M; g.Hd = Hd; g.vecA = 1; g.vecB = 1;
    const Lstm16 x = {w_h_bf16, dgates_next_bf16, dgates_bf16, dgx_bf16};
    hipLaunchKernelGGL(lstm_bwd_wide16_kernel, dim3(air_cdiv(M, 16) * (Hd / 64)), dim3(512), 0, air_stream(stream), g, x);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

template <bool BF>
static int lstm_fwd_launch(const LstmFwdArgs &g, const PrologueArgs &pro, int extra_blocks, hipStream_t st) {
    // more than 512 16x16 tiles of (batch, hidden): the wide-tile form (needs 16-byte addressable operands and Hd % 64 == 0)
    const bool wide = air_cdiv(g.M, 16) * air_cdiv(g.Hd, 16) > 512 && g.Hd % 64 == 0 && g.ldw % 4 == 0 && g.ldh % 4 == 0 &&
                      air_aligned16(g.w_h) && air_aligned16(g.h_prev);
    if (wide) {
        LstmFwdArgs gw = g;
        gw.tiles = air_cdiv(g.M, 16) * (g.Hd / 64);
        hipLaunchKernelGGL((lstm_fwd_wide_kernel<BF>), dim3(gw.tiles + extra_blocks), dim3(512), 0, st, gw, pro);
    } else {
        hipLaunchKernelGGL((lstm_fwd_fused_kernel<BF>), dim3(g.tiles + extra_blocks), dim3(256), 0, st, g, pro);
    }
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
static int lstm_fwd_fill(LstmFwdArgs &g, const float *h_prev, int ldh, const float *c_prev, int ldc, const float *w_h,
                         int ldw, const float *gx, int ldgx, float *h, float *c, float *gate_act, int M, int Hd,
                         float forget_bias, int precision) {
    AIR_REQUIRE(h_prev && c_prev && w_h && gx && h && c && gate_act, AIR_E_NULL);
    AIR_REQUIRE(M > 0 && Hd > 0 && ldw >= 4 * Hd && ldgx >= 4 * Hd, AIR_E_SHAPE);
    AIR_REQUIRE((ldh == 0 || ldh >= Hd) && (ldc == 0 || ldc >= Hd), AIR_E_SHAPE);
    AIR_REQUIRE(precision == AIR_PREC_F32 || precision == AIR_PREC_BF16, AIR_E_UNSUPPORTED);
    g.h_prev = h_prev; g.w_h = w_h; g.gx = gx; g.c_prev = c_prev; g.h = h; g.c = c; g.gate_act = gate_act;
    g.M = M; g.Hd = Hd; g.ldw = ldw; g.ldgx = ldgx; g.fb = forget_bias; g.ldh = ldh; g.ldc = ldc;
    g.vecA = ((ldh % 4) == 0 && air_aligned16(h_prev)) ? 1 : 0;
    g.tiles = air_cdiv(M, 16) * air_cdiv(Hd, 4);
    return AIR_OK;
}
extern "C" int air_lstm_step_fwd(const float *h_prev, const float *c_prev, const float *w_h, int ldw, const float *gx,
                                 int ldgx, float *h, float *c, float *gate_act, int M, int Hd, float forget_bias,
                                 int precision, void *stream) {
    LstmFwdArgs g;
    int st = lstm_fwd_fill(g, h_prev, Hd, c_prev, Hd, w_h, ldw, gx, ldgx, h, c, gate_act, M, Hd, forget_bias, precision);
    if (st) return st;
    PrologueArgs pro = {};
    return precision == AIR_PREC_BF16 ? lstm_fwd_launch<true>(g, pro, 0, air_stream(stream))
                                      : lstm_fwd_launch<false>(g, pro, 0, air_stream(stream));
}
// First LSTM step of a train step with the step prologue riding along: h0 / c0 [1,Hd] are read with a broadcast row stride
// by the step itself, while extra workgroups draw the step's noise, evaluate the annealed prior and write the tiled
// initial state (needed only by later launches: the backward reads h_tiled / c_tiled).
extern "C" int air_lstm_step_fwd_prologue(const float *h0, const float *c0, const float *w_h, int ldw, const float *gx,
                                          int ldgx, float *h, float *c, float *gate_act, int M, int Hd, float forget_bias,
                                          int precision, float *normal, size_t n_normal, float *uniform, size_t n_uniform,
                                          const uint64_t *rng_state_dev, const int64_t *global_step_dev, int anneal_type,
                                          double init, double final_value, double anneal_steps, double hold_for,
                                          double steps_div, double *prior_out_f64, int T, float *h_tiled, float *c_tiled,
                                          void *stream) {
    AIR_REQUIRE(rng_state_dev && global_step_dev && prior_out_f64 && h_tiled && c_tiled, AIR_E_NULL);
    AIR_REQUIRE((n_normal == 0 || normal) && (n_uniform == 0 || uniform), AIR_E_NULL);
    AIR_REQUIRE(T > 0 && anneal_type >= 0 && anneal_type <= 2, AIR_E_SHAPE);
    LstmFwdArgs g;
    int st = lstm_fwd_fill(g, h0, 0, c0, 0, w_h, ldw, gx, ldgx, h, c, gate_act, M, Hd, forget_bias, precision);
    if (st) return st;
    const PrologueArgs pro = make_prologue_args(normal, n_normal, uniform, n_uniform, rng_state_dev, global_step_dev,
                                                anneal_type, init, final_value, anneal_steps, hold_for, steps_div,
                                                prior_out_f64, T, h0, c0, h_tiled, c_tiled, M, Hd);
    const int extra = prologue_blocks(pro);
    return precision == AIR_PREC_BF16 ? lstm_fwd_launch<true>(g, pro, extra, air_stream(stream))
                                      : lstm_fwd_launch<false>(g, pro, extra, air_stream(stream));
}

// air_lstm_step_fwd_prologue with the hoisted input product x . W_x + b folded in (lstm_fwd_first_kernel): latency regime only --
// AIR_E_UNSUPPORTED beyond 512 tiles of (batch, hidden) and where the gx product alone would leave the 4-wave 16x16 body: the caller
// keeps the gx launch and the first step with the prologue there.
extern "C" int air_lstm_first_step_fwd(const float *x, int ldx, int E, const float *w_x, const float *b_gates, const float *h0,
                                       const float *c0, const float *w_h, int ldw, float *gx_out, int ldgx, float *h, float *c,
                                       float *gate_act, int M, int Hd, float forget_bias, int precision, float *normal,
                                       size_t n_normal, float *uniform, size_t n_uniform, const uint64_t *rng_state_dev,
                                       const int64_t *global_step_dev, int anneal_type, double init, double final_value,
                                       double anneal_steps, double hold_for, double steps_div, double *prior_out_f64, int T,
                                       float *h_tiled, float *c_tiled, void *stream) {
    AIR_REQUIRE(x && w_x && b_gates && gx_out, AIR_E_NULL);
    AIR_REQUIRE(rng_state_dev && global_step_dev && prior_out_f64 && h_tiled && c_tiled, AIR_E_NULL);
    AIR_REQUIRE((n_normal == 0 || normal) && (n_uniform == 0 || uniform), AIR_E_NULL);
    AIR_REQUIRE(T > 0 && anneal_type >= 0 && anneal_type <= 2 && E > 0 && ldx >= E, AIR_E_SHAPE);
    AIR_REQUIRE(air_cdiv(M, 16) * air_cdiv(Hd, 16) <= 512, AIR_E_UNSUPPORTED);
    // The kernel repeats the K order of the 4-wave 16x16 body, so it takes the shapes whose gx product [M, 4Hd, E] air_gemm_grouped runs
    // on that body as a launch of its own.  Beyond (more than wide_min_tiles() tiles of gx: the wide-tile kernels or 32x32 tiles; a long
    // K: the 16-wave split) the two launches it replaces give other bits -- found at M = 512, Hd = 256, E = 52 with bf16 operands, where
    // 22 358 of 526 336 elements of gx differed -- and the caller keeps them.
    AIR_REQUIRE(air_gemm_lone_on_tile16_kw4(M, 4 * Hd, E), AIR_E_UNSUPPORTED);
    LstmFwdArgs g;
    int st = lstm_fwd_fill(g, h0, 0, c0, 0, w_h, ldw, gx_out, ldgx, h, c, gate_act, M, Hd, forget_bias, precision);
    if (st) return st;
    LstmFirstArgs f;
    f.x = x; f.w_x = w_x; f.b = b_gates; f.gx_out = gx_out; f.E = E; f.ldx = ldx;
    f.vecX = ((ldx % 4) == 0 && air_aligned16(x)) ? 1 : 0;
    const PrologueArgs pro = make_prologue_args(normal, n_normal, uniform, n_uniform, rng_state_dev, global_step_dev,
                                                anneal_type, init, final_value, anneal_steps, hold_for, steps_div,
                                                prior_out_f64, T, h0, c0, h_tiled, c_tiled, M, Hd);
    const int extra = prologue_blocks(pro);
    if (precision == AIR_PREC_BF16)
        hipLaunchKernelGGL((lstm_fwd_first_kernel<true>), dim3(g.tiles + extra), dim3(256), 0, air_stream(stream), g, f, pro);
    else
        hipLaunchKernelGGL((lstm_fwd_first_kernel<false>), dim3(g.tiles + extra), dim3(256), 0, air_stream(stream), g, f, pro);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ---- the owned tile shape of the 16-wave BPTT kernels (lstm_bwd_fused_kernel<16, false, R, C>, lstm_bwd_entry_kernel<R, C>) ----------
// AIR_LSTM_BWD_TILE (air_common.h: air_tile_env; the launches' names there are "link" and "entry").  A forced shape the entry point
// cannot honour -- the 4-wave or wide-tile link, bf16 operands, a value the switch does not know -- is AIR_E_UNSUPPORTED before anything
// is launched.
// auto: half tiles where the 16x16 tiling leaves at least half the CUs without a tile and K = 4 Hd >= 512 (below, a tile's operands
// are no more than a forward step's and the launch sits on its floor) -- the shape each launch's own A/B adopted
// (profiles/half_tiles_ab.txt: 8x16 for both, with the optimiser riders aboard; 8x8, a tile on every CU, LOST 2-3 us per launch).
enum { LSTM_LINK_TILE = AIR_TILE_8x16, LSTM_ENTRY_TILE = AIR_TILE_8x16 };
static int lstm_bwd_tile_auto(int M, int Hd, int adopted) {
    const long tiles16 = (long)air_cdiv(M, 16) * air_cdiv(Hd, 16);
    return (2 * tiles16 > air_cu_count() || 4 * Hd < 512) ? (int)AIR_TILE_16x16 : adopted;
}

template <bool BF>
static int lstm_bwd_launch(const LstmBwdArgs &g, const RmspropSlice &opt, size_t opt_nq, hipStream_t st) {
    const int tiles = air_cdiv(g.M, 16) * air_cdiv(g.Hd, 16);
    // few tiles (batch 64: 64 of them): 16 waves share the 4Hd-deep contraction of a tile; many tiles: 4 waves
    const bool wide = tiles > 512 && g.Hd % 64 == 0 && g.vecA && g.vecB;
    const int nth = tiles <= 512 ? 1024 : (wide ? 512 : 256);
    size_t extra = air_rider_blocks(opt_nq, nth, 512);                     // about two float4 per thread of the riding slice
    int shape = air_tile_env("AIR_LSTM_BWD_TILE", "link");
    AIR_REQUIRE(shape != AIR_TILE_UNKNOWN, AIR_E_UNSUPPORTED);
    AIR_REQUIRE(shape == AIR_TILE_AUTO || shape == AIR_TILE_16x16 || (tiles <= 512 && !BF), AIR_E_UNSUPPORTED);
    if (shape == AIR_TILE_AUTO)
        shape = (tiles <= 512 && !BF) ? lstm_bwd_tile_auto(g.M, g.Hd, LSTM_LINK_TILE) : AIR_TILE_16x16;
    if (wide) hipLaunchKernelGGL((lstm_bwd_wide_kernel<BF>), dim3(air_cdiv(g.M, 16) * (g.Hd / 64) + (int)extra), dim3(512), 0, st, g, opt);
    else if (shape == AIR_TILE_8x16)
        hipLaunchKernelGGL((lstm_bwd_fused_kernel<16, false, 8, 16>), dim3(air_cdiv(g.M, 8) * air_cdiv(g.Hd, 16) + (int)extra), dim3(1024), 0, st, g, opt);
    else if (shape == AIR_TILE_8x8)
        hipLaunchKernelGGL((lstm_bwd_fused_kernel<16, false, 8, 8>), dim3(air_cdiv(g.M, 8) * air_cdiv(g.Hd, 8) + (int)extra), dim3(1024), 0, st, g, opt);
    else if (tiles <= 512) hipLaunchKernelGGL((lstm_bwd_fused_kernel<16, BF>), dim3(tiles + (int)extra), dim3(1024), 0, st, g, opt);
    else hipLaunchKernelGGL((lstm_bwd_fused_kernel<4, BF>), dim3(tiles + (int)extra), dim3(256), 0, st, g, opt);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
extern "C" int air_lstm_step_bwd(const float *dgates_next, const float *w_h, const float *dh_a, const float *dh_b,
                                 const float *dc_in, const float *gate_act, const float *c_prev, const float *c,
                                 const float *dgx_in, float *dgates, float *dc_prev, float *dgx_out, int M, int Hd,
                                 int precision, void *stream) {
    return air_lstm_step_bwd_opt(dgates_next, w_h, dh_a, dh_b, dc_in, gate_act, c_prev, c, dgx_in, dgates, dc_prev, dgx_out, M,
                                 Hd, precision, nullptr, stream);
}
extern "C" int air_lstm_step_bwd_opt(const float *dgates_next, const float *w_h, const float *dh_a, const float *dh_b,
                                     const float *dc_in, const float *gate_act, const float *c_prev, const float *c,
                                     const float *dgx_in, float *dgates, float *dc_prev, float *dgx_out, int M, int Hd,
                                     int precision, const AirRmspropSlice *opt, void *stream) {
    RmspropSlice os; size_t onq;
    { int st_ = rmsprop_slice_from_abi(opt, os, &onq); if (st_) return st_; }
    AIR_REQUIRE(dgates_next && w_h && gate_act && c_prev && c && dgates && dc_prev, AIR_E_NULL);
    AIR_REQUIRE(M > 0 && Hd > 0, AIR_E_SHAPE);
    AIR_REQUIRE(precision == AIR_PREC_F32 || precision == AIR_PREC_BF16, AIR_E_UNSUPPORTED);
    LstmBwdArgs g;
    g.dgates_next = dgates_next; g.w_h = w_h; g.dh_a = dh_a; g.dh_b = dh_b; g.dc_in = dc_in; g.gate_act = gate_act;
    g.c_prev = c_prev; g.c = c; g.dgx_in = dgx_in; g.dgates = dgates; g.dc_prev = dc_prev; g.dgx_out = dgx_out;
    g.M = M; g.Hd = Hd;
    g.vecA = air_aligned16(dgates_next) ? 1 : 0;          // row stride 4*Hd floats is always a multiple of 16 bytes
    g.vecB = air_aligned16(w_h) ? 1 : 0;
    return precision == AIR_PREC_BF16 ? lstm_bwd_launch<true>(g, os, onq, air_stream(stream))
                                      : lstm_bwd_launch<false>(g, os, onq, air_stream(stream));
}

extern "C" int air_lstm_step_bwd_entry_fits(int M, int Hd) {
    return (M > 0 && Hd > 0 && Hd % 16 == 0 && air_cdiv(M, 16) * (Hd / 16) <= 512) ? 1 : 0;
}
extern "C" int air_lstm_step_bwd_entry(const float *gate_act1, const float *c_prev1, const float *c1, const float *dh_a1,
                                       const float *dh_b1, float *dgates1, float *dc_prev1, const float *w_h, const float *dh_a,
                                       const float *dh_b, const float *gate_act, const float *c_prev, const float *c, float *dgates,
                                       float *dc_prev, float *dgx_out, int M, int Hd, const AirRmspropSlice *opt, void *stream) {
    RmspropSlice os; size_t onq;
    { int st_ = rmsprop_slice_from_abi(opt, os, &onq); if (st_) return st_; }
    AIR_REQUIRE(gate_act1 && c_prev1 && c1 && dgates1 && dc_prev1 && w_h && gate_act && c_prev && c && dgates && dc_prev, AIR_E_NULL);
    AIR_REQUIRE(dh_a1 || dh_b1, AIR_E_NULL);
    AIR_REQUIRE(air_lstm_step_bwd_entry_fits(M, Hd) == 1, AIR_E_UNSUPPORTED);
    // (Hd % 16 == 0: every row of every operand is a multiple of 64 bytes; the bases must be 16-byte aligned)
    AIR_REQUIRE(air_aligned16(gate_act1) && air_aligned16(c_prev1) && air_aligned16(c1) && air_aligned16(dgates1) &&
                air_aligned16(dc_prev1) && air_aligned16(w_h) && (!dh_a1 || air_aligned16(dh_a1)) && (!dh_b1 || air_aligned16(dh_b1)),
                AIR_E_ALIGN);
    LstmBwdArgs g;
    g.dgates_next = dgates1; g.w_h = w_h; g.dh_a = dh_a; g.dh_b = dh_b; g.dc_in = nullptr; g.gate_act = gate_act;
    g.c_prev = c_prev; g.c = c; g.dgx_in = nullptr; g.dgates = dgates; g.dc_prev = dc_prev; g.dgx_out = dgx_out;
    g.M = M; g.Hd = Hd; g.vecA = 1; g.vecB = 1;
    LstmEntryArgs en;
    en.gate_act1 = gate_act1; en.c_prev1 = c_prev1; en.c1 = c1; en.dh_a1 = dh_a1; en.dh_b1 = dh_b1; en.dgates1 = dgates1;
    en.dc_prev1 = dc_prev1;
    size_t extra = air_rider_blocks(onq, 1024, 512);
    int shape = air_tile_env("AIR_LSTM_BWD_TILE", "entry");
    AIR_REQUIRE(shape != AIR_TILE_UNKNOWN, AIR_E_UNSUPPORTED);
    if (shape == AIR_TILE_AUTO) shape = lstm_bwd_tile_auto(M, Hd, LSTM_ENTRY_TILE);
    if (shape == AIR_TILE_8x16)
        hipLaunchKernelGGL((lstm_bwd_entry_kernel<8, 16>), dim3(air_cdiv(M, 8) * (Hd / 16) + (int)extra), dim3(1024), 0, air_stream(stream), g, en, os);
    else if (shape == AIR_TILE_8x8)
        hipLaunchKernelGGL((lstm_bwd_entry_kernel<8, 8>), dim3(air_cdiv(M, 8) * (Hd / 8) + (int)extra), dim3(1024), 0, air_stream(stream), g, en, os);
    else
        hipLaunchKernelGGL((lstm_bwd_entry_kernel<16, 16>), dim3(air_cdiv(M, 16) * (Hd / 16) + (int)extra), dim3(1024), 0, air_stream(stream), g, en, os);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
