// Exact subset MAP of a scene parse for gfx950: which of the T computed steps (T <= 6: at most 64 subsets) to keep.
//   air_prune_score:   per image, row band and subset mask m the band's share of the reconstruction term of
//                      canvas_m = sum_{t in m} st_write(glimpse_t, where_t) against obs -- one pass over the pixels for all masks;
//   air_prune_select:  per image the latent terms of every step, the joint J_m = log p(x, z_m) of every mask in float64, the arg-max
//                      under the visiting rule (the start mask first, then from the full mask down; strict), the evidence of every
//                      candidate step, and the rows of the parse compacted into a leading-ones chain (a stable partition, bit copies);
//   air_prune_relabel: score / obj_score / obj_step of the kept rows behind air_parse_objects, which labels rows by position.
// No atomics, no cross-workgroup traffic; every sum has one fixed order: the same bits run to run.
#include <math.h>
#include "scene_device.h"

#define PRUNE_MAXT 6
#define PRUNE_THREADS 256

// ============================================================================================================
// score
// ============================================================================================================
// behind the common head of the carve: the presence row (8 floats), then (PRUNE_THREADS / 64) * 2^T wave totals
static inline size_t prune_tail_floats(int T) { return 8 + (size_t)(PRUNE_THREADS / 64) * (1u << T); }
struct PruneScoreArgs {
    const float *glimpse, *where, *presence, *obs;
    float *rec_sub;
    int B, NB, RB, H, W, h, w;
    double stepX, stepY;
    float mult, std;
    int all_candidates, vec4_glimpse;
};

// canvas of mask M from the register-held layers: 0 + the set bits' layers in step order (the adds of parse_render_kernel for a
// presence row equal to the mask's bits)
template <int T, int M>
__device__ __forceinline__ float prune_canvas(const float (&v)[T]) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t)
        if ((M >> t) & 1) acc = acc + v[t];
    return acc;
}
// the mask loop, unrolled at compile time: accumulator M is a register of its own (a runtime-indexed array would live in scratch)
template <int T, int M>
struct PruneMasks {
    static __device__ __forceinline__ void add(const float (&v)[T], float (&s)[1 << T], float x, float mult, float std, float cst) {
#pragma clang fp contract(off)
        const float rc = mult * prune_canvas<T, M>(v);
        const float z = (x - rc) / std;
        s[M] += 0.5f * z * z + cst;
        PruneMasks<T, M + 1>::add(v, s, x, mult, std, cst);
    }
    static __device__ __forceinline__ void fold(float (&s)[1 << T], float *scratch, int wid, int lane) {
        const float tot = wave_sum_all(s[M]);
        if (lane == 0) scratch[wid * (1 << T) + M] = tot;
        PruneMasks<T, M + 1>::fold(s, scratch, wid, lane);
    }
};
template <int T>
struct PruneMasks<T, 1 << T> {
    static __device__ __forceinline__ void add(const float (&)[T], float (&)[1 << T], float, float, float, float) {}
    static __device__ __forceinline__ void fold(float (&)[1 << T], float *, int, int) {}
};

// One workgroup per (image, row band), air_canvas_unroll_bands' banding, parse_render_kernel's staging: every global operand is
// requested up front, ONE barrier, then each thread walks its pixels (p = tid, tid + nt, ...) with the T layer values and the 2^T
// accumulators in registers.  A step t >= c_b (c_b = n_b, or T with all_candidates) contributes a layer of exactly 0 -- a
// workgroup-uniform select, no divergence on n_b.  The band's sums: a butterfly inside each wave, the four wave totals through LDS,
// added in wave order by thread m.
template <int T>
__global__ __launch_bounds__(PRUNE_THREADS) void prune_score_kernel(PruneScoreArgs a) {
#pragma clang fp contract(off)
    constexpr int NM = 1 << T;
    extern __shared__ __align__(16) float smem[];
    const float *__restrict__ glimpse = a.glimpse, *__restrict__ where = a.where, *__restrict__ presence = a.presence;
    const float *__restrict__ obs = a.obs;
    const int B = a.B, RB = a.RB, H = a.H, W = a.W, h = a.h, w = a.w;
    const float mult = a.mult, std = a.std;
    const int HW = H * W, tid = threadIdx.x, nt = PRUNE_THREADS, lane = tid & 63, wid = tid >> 6;
    const BandCarve c = band_carve(smem, T, RB, W, h, w);
    float *pres = c.tail, *scratch = c.tail + 8;
    const float cst = 0.5f * logf(6.283185307179586f) + logf(std);
    const int pitch = w + 2;
    const float inv_W = 1.0f / (float)W;
    const int unit = blockIdx.x;                                   // < B * NB: the grid is exactly the units
    const int b = unit % B, band = unit / B;
    const int r0 = band * RB, r1 = (r0 + RB < H) ? r0 + RB : H, npx = (r1 - r0) * W, pbase = r0 * W;
    const float *ob = obs + (size_t)b * HW + pbase;
    const int ob_last = npx - 1;
    // ---- every global load of this unit ----------------------------------------------------------------------------------
    float xo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xo[u] = band_prefetch_obs(ob, ob_last, tid + u * nt);
    band_zero_borders(c, T, h, w, tid, nt);
    band_stage_glimpses(c, glimpse, a.vec4_glimpse != 0, T, B, b, h, w, tid, nt);
    band_axis_tables(c, where, T, B, b, RB, H, W, h, w, r0, r1 - r0, a.stepX, a.stepY, tid, nt);
    if (tid < T) pres[tid] = presence[(size_t)tid * B + b];
    __syncthreads();
    int cb = T;                                                    // candidates: workgroup-uniform
    if (!a.all_candidates) {
        cb = 0;
        while (cb < T && pres[cb] > 0.5f) ++cb;                  // leading ones
    }
    float s[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) s[m] = 0.f;
    for (int base = 0; base < npx; base += 4 * nt) {
        float xn[4] = {0.f, 0.f, 0.f, 0.f};
        if (base + 4 * nt < npx) {                                 // next chunk's observations (bands above 4 pixels per thread)
#pragma unroll
            for (int u = 0; u < 4; ++u) xn[u] = band_prefetch_obs(ob, ob_last, base + tid + (4 + u) * nt);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = base + tid + u * nt;
            if (p < npx) {
                const int Ib = div_small(p, W, inv_W), J = p - Ib * W;
                float v[T];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float2 ex = c.xe[t * W + J], ey = c.ye[t * RB + Ib];
                    const int fx = __float_as_int(ex.x), fy = __float_as_int(ey.x);
                    float val = 0.f;
                    if (t < cb && fx != ST_INVALID && fy != ST_INVALID)
                        val = bilerp(load_taps_pad(c.glm + (size_t)t * c.hwp, pitch, fy, fx), ex.y, ey.y);
                    v[t] = val;
                }
                PruneMasks<T, 0>::add(v, s, xo[u], mult, std, cst);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xo[u] = xn[u];
    }
    PruneMasks<T, 0>::fold(s, scratch, wid, lane);
    __syncthreads();
    if (tid < (1 << cb)) {                                         // only the masks over the candidates are written
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < PRUNE_THREADS / 64; ++k) tot += scratch[k * NM + tid];
        a.rec_sub[((size_t)band * B + b) * NM + tid] = tot;
    }
}

extern "C" int air_prune_score(const float *glimpse, const float *where, const float *presence, const float *obs, float mult,
                               float std, int all_candidates, int T, int R, int H, int W, int h, int w, int n_bands,
                               float *rec_sub, void *stream) {
    AIR_REQUIRE(glimpse && where && presence && obs && rec_sub, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= PRUNE_MAXT && R > 0 && H > 0 && W > 0 && h > 0 && w > 0 && n_bands > 0, AIR_E_SHAPE);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(presence) |
                           reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(rec_sub);
    int NB, RB;
    size_t lds;                                                    // (n_bands: the caller sized rec_sub for exactly these shares)
    { int st_ = band_launch_prepare(T, R, H, W, h, w, n_bands, where, bits, prune_tail_floats(T), &NB, &RB, &lds); if (st_) return st_; }
    const PruneScoreArgs a = {glimpse, where, presence, obs, rec_sub, R, NB, RB, H, W, h, w, lin_step(W), lin_step(H), mult, std,
                              all_candidates != 0, (w % 4 == 0) && air_aligned16(glimpse)};
    const dim3 grid((unsigned)((long)R * NB)), block(PRUNE_THREADS);
#define PRUNE_LAUNCH(TT)                                                                             \
    case TT: {                                                                                       \
        int st_ = cv_allow_lds(prune_score_kernel<TT>, lds);                                         \
        if (st_) return st_;                                                                         \
        hipLaunchKernelGGL(prune_score_kernel<TT>, grid, block, lds, air_stream(stream), a);         \
    } break
    switch (T) {
        PRUNE_LAUNCH(1); PRUNE_LAUNCH(2); PRUNE_LAUNCH(3); PRUNE_LAUNCH(4); PRUNE_LAUNCH(5); PRUNE_LAUNCH(6);
    }
#undef PRUNE_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// select
// ============================================================================================================
struct PrunePriors {
    float what_loc, what_scale, scale_loc, scale_scale, shift_loc, shift_scale;   // shift_loc NaN: centred on where_loc
};

struct PruneSelectArgs {
    const float *what, *where, *glimpse, *score, *presence, *where_loc, *rec_sub;
    const double *prior;
    PrunePriors pr;
    int normalize, all_candidates, n_bands, T, R, A, G, what_vec, glimpse_vec;
    double *J_sub, *objective, *objective_start, *evidence;
    int *best_mask, *num_objects_out, *kept_step;
    float *what_out, *where_out, *glimpse_out, *score_out;
};

// One wavefront per image.  The latent term of step t: the lanes stride over the A / V vectors of the step's `what` row (items in
// index order), lane 0 adds the four `where` terms of the step behind its items, a butterfly adds the lanes -- the same layout for
// every step, so two steps with the same latents have the same term bit for bit.  Lane m then owns
// mask m (2^T <= 64): band shares in band order, the set steps' terms in step order, log pi(popcount m), all closing adds in
// float64.  The arg-max is a butterfly under a symmetric rule -- the larger J, between equal J the earlier visit -- so every lane
// ends with the same mask: what the sequential visit with its strict comparison gives.
template <int V>
__global__ __launch_bounds__(256) void prune_select_kernel(PruneSelectArgs a) {
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int T = a.T, R = a.R, A = a.A, G = a.G;
    if (r >= R) return;                                            // wave-uniform
    const int NM = 1 << T;
    const float z = lane < T ? a.presence[(size_t)lane * R + r] : 0.f;
    const unsigned long long present = __ballot(z > 0.5f);         // lanes >= T are clear: ~present is never 0
    const int n = __ffsll((long long)~present) - 1;
    const int cb = a.all_candidates ? T : n;
    const int m0 = (1 << n) - 1;
    const PrunePriors pr = a.pr;
    const bool centred = pr.shift_loc != pr.shift_loc;

    // ---- latent terms ---------------------------------------------------------------------------------------------------
    const float log_pw = logf(pr.what_scale), log_ps = logf(pr.scale_scale), log_ph = logf(pr.shift_scale);
    const int AV = A / V;
    double lp[PRUNE_MAXT];
#pragma unroll
    for (int t = 0; t < PRUNE_MAXT; ++t) {
        lp[t] = 0.0;
        if (t < cb) {                                              // wave-uniform
            float s = 0.f;
            const size_t row = (size_t)t * R + r;
            for (int i = lane; i < AV; i += 64) {
                const vec_t x = *reinterpret_cast<const vec_t *>(a.what + row * A + (size_t)i * V);
                const float *xf = reinterpret_cast<const float *>(&x);
#pragma unroll
                for (int v = 0; v < V; ++v) s += log_normal(xf[v], pr.what_loc, pr.what_scale, log_pw);
            }
            if (lane == 0) {
                const float4 x = *reinterpret_cast<const float4 *>(a.where + row * 4);
                float ly = pr.shift_loc, lw = pr.shift_loc;
                if (centred) {
                    const float4 l = *reinterpret_cast<const float4 *>(a.where_loc + row * 4);
                    ly = l.y; lw = l.w;
                }
                s += log_normal(x.x, pr.scale_loc, pr.scale_scale, log_ps);
                s += log_normal(x.y, ly, pr.shift_scale, log_ph);
                s += log_normal(x.z, pr.scale_loc, pr.scale_scale, log_ps);
                s += log_normal(x.w, lw, pr.shift_scale, log_ph);
            }
            lp[t] = (double)wave_sum_all(s);
        }
    }

    // ---- the joint of mask m = lane ---------------------------------------------------------------------------------------
    const int m = lane;
    const bool live = m < (1 << cb);
    double J = __longlong_as_double(0x7ff8000000000000LL);
    if (live) {
        float rec = 0.f;                                           // the operations of air_sum_leading
        for (int k = 0; k < a.n_bands; ++k) rec += a.rec_sub[((size_t)k * R + r) * NM + m];
        double lat = 0.0;
#pragma unroll
        for (int t = 0; t < PRUNE_MAXT; ++t)
            if ((m >> t) & 1) lat += lp[t];
        double total = 1.0;
        if (a.normalize) {
            total = 0.0;
            for (int i = 0; i <= T; ++i) total += a.prior[i];
        }
        J = (-(double)rec + lat) + log(a.prior[__popc((unsigned)m)] / total);
    }
    if (m < NM) a.J_sub[(size_t)r * NM + m] = J;

    // ---- selection: m0 first, then 2^c - 1 down to 0; strict ------------------------------------------------------------
    double best = J;
    int bm = m, have = (live && J == J) ? 1 : 0;
    int rank = m == m0 ? 0 : 1 + ((1 << cb) - 1 - m);              // position in the visiting order (unique among the live masks)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(best, off, 64);
        const int om = __shfl_xor(bm, off, 64), oh = __shfl_xor(have, off, 64), ork = __shfl_xor(rank, off, 64);
        if (oh && (!have || os > best || (os == best && ork < rank))) { best = os; bm = om; rank = ork; have = 1; }
    }
    if (!have) bm = m0;                                            // everything NaN: the parse stays
    const double J0 = __shfl(J, m0, 64);
    const double Jb = __shfl(J, bm, 64);
    const int kept = __popc((unsigned)bm);
    // evidence of step t = lane: J(m0 with bit t) - J(m0 without it)
    {
        const int t = lane < T ? lane : 0;
        const double with = __shfl(J, m0 | (1 << t), 64), without = __shfl(J, m0 & ~(1 << t), 64);
        if (lane < T) a.evidence[(size_t)lane * R + r] = lane < cb ? with - without : __longlong_as_double(0x7ff8000000000000LL);
    }
    // stable partition: output row j = the j-th kept step, then the (j - kept)-th other step
    int src = 0;
    if (lane < T) {
        const int want_set = lane < kept ? 1 : 0;
        int k = lane < kept ? lane : lane - kept;
        for (int t = 0; t < T; ++t) {
            if (((bm >> t) & 1) == want_set) {
                if (k == 0) src = t;
                --k;
            }
        }
        a.kept_step[(size_t)lane * R + r] = src;
    }
    if (lane == 0) {
        a.best_mask[r] = bm;
        a.num_objects_out[r] = kept;
        a.objective[r] = Jb;
        a.objective_start[r] = J0;
    }
    for (int j = 0; j < T; ++j) {                                  // bit copies of all T rows of this image
        const int t = __shfl(src, j, 64);
        const size_t from = (size_t)t * R + r, to = (size_t)j * R + r;
        if (lane < 4) reinterpret_cast<unsigned *>(a.where_out)[to * 4 + lane] = reinterpret_cast<const unsigned *>(a.where)[from * 4 + lane];
        if (lane == 4) reinterpret_cast<unsigned *>(a.score_out)[to] = reinterpret_cast<const unsigned *>(a.score)[from];
        copy_row_bits(a.what + from * A, a.what_out + to * A, A, a.what_vec != 0, lane);
        copy_row_bits(a.glimpse + from * G, a.glimpse_out + to * G, G, a.glimpse_vec != 0, lane);
    }
}

extern "C" int air_prune_select(const float *what, const float *where, const float *glimpse, const float *score, const float *presence,
                                const float *where_loc, float what_p_loc, float what_p_scale, float scale_p_loc, float scale_p_scale,
                                float shift_p_loc, float shift_p_scale, const double *prior_f64, int normalize_prior,
                                int all_candidates, const float *rec_sub, int n_bands, int T, int R, int A, int G, double *J_sub,
                                int *best_mask, int *num_objects_out, int *kept_step, double *objective, double *objective_start,
                                double *evidence, float *what_out, float *where_out, float *glimpse_out, float *score_out,
                                void *stream) {
    AIR_REQUIRE(what && where && glimpse && score && presence && prior_f64 && rec_sub && J_sub && best_mask && num_objects_out &&
                kept_step && objective && objective_start && evidence && what_out && where_out && glimpse_out && score_out, AIR_E_NULL);
    AIR_REQUIRE(shift_p_loc == shift_p_loc || where_loc, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= PRUNE_MAXT && R > 0 && A > 0 && G > 0 && n_bands > 0, AIR_E_SHAPE);
    AIR_REQUIRE(n_bands <= 8, AIR_E_SHAPE);                       // the most air_canvas_unroll_bands returns: rec_sub is [n_bands, R, 2^T]
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_loc) && air_aligned16(where_out), AIR_E_ALIGN);
    const uintptr_t all = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(score) |
                          reinterpret_cast<uintptr_t>(presence) | reinterpret_cast<uintptr_t>(rec_sub) |
                          reinterpret_cast<uintptr_t>(best_mask) | reinterpret_cast<uintptr_t>(num_objects_out) |
                          reinterpret_cast<uintptr_t>(kept_step) | reinterpret_cast<uintptr_t>(what_out) |
                          reinterpret_cast<uintptr_t>(glimpse_out) | reinterpret_cast<uintptr_t>(score_out);
    const uintptr_t dbl = reinterpret_cast<uintptr_t>(prior_f64) | reinterpret_cast<uintptr_t>(J_sub) | reinterpret_cast<uintptr_t>(objective) |
                          reinterpret_cast<uintptr_t>(objective_start) | reinterpret_cast<uintptr_t>(evidence);
    AIR_REQUIRE((all & 3u) == 0 && (dbl & 7u) == 0, AIR_E_ALIGN);
    const PrunePriors pr = {what_p_loc, what_p_scale, scale_p_loc, scale_p_scale, shift_p_loc, shift_p_scale};
    const PruneSelectArgs a = {what, where, glimpse, score, presence, where_loc, rec_sub, prior_f64, pr, normalize_prior != 0,
                               all_candidates != 0, n_bands, T, R, A, G,
                               A % 4 == 0 && air_aligned16(what) && air_aligned16(what_out),
                               G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(glimpse_out),
                               J_sub, objective, objective_start, evidence, best_mask, num_objects_out, kept_step,
                               what_out, where_out, glimpse_out, score_out};
    const uintptr_t wbits = reinterpret_cast<uintptr_t>(what);
    const dim3 grid(air_cdiv(R, 4)), block(256);
#define PN_LAUNCH(V) hipLaunchKernelGGL(prune_select_kernel<V>, grid, block, 0, air_stream(stream), a)
    if (A % 4 == 0 && (wbits & 15u) == 0) PN_LAUNCH(4);
    else if (A % 2 == 0 && (wbits & 7u) == 0) PN_LAUNCH(2);
    else PN_LAUNCH(1);
#undef PN_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// relabel
// ============================================================================================================
// The kernel is parse_relabel_kernel (parse_kernels.hip); this entry stops at the steps subset pruning enumerates.
extern "C" int air_prune_relabel(const float *score_src, const int *kept_step, const int *num_objects, const int *offsets, int T,
                                 int R, float *score, float *obj_score, int *obj_step, void *stream) {
    AIR_REQUIRE(score_src && kept_step && num_objects && offsets && score && obj_score && obj_step, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= PRUNE_MAXT && R > 0, AIR_E_SHAPE);
    const uintptr_t all = reinterpret_cast<uintptr_t>(score_src) | reinterpret_cast<uintptr_t>(kept_step) |
                          reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(offsets) |
                          reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(obj_score) | reinterpret_cast<uintptr_t>(obj_step);
    AIR_REQUIRE((all & 3u) == 0, AIR_E_ALIGN);
    return parse_relabel_launch(score_src, kept_step, num_objects, offsets, T, R, score, obj_score, obj_step, stream);
}
