// Proposing missed objects from the residual image behind a scene parse, for gfx950 (include/air_hip.h states the rules):
//   air_propose_residual: res = clamp(obs - mult * canvas of the rows t < n_b) -- the image the inference network is shown again.
//                         parse_render_kernel's staging and per-pixel operations (so the canvas has air_parse_render's bits), but it
//                         writes the residual and the optional band shares of sum res^2 and nothing else: no owner map, no areas,
//                         no reconstruction;
//   air_propose_pool:     the candidate pool of C = T + P rows per image: the T current rows followed by P proposal rows (bit
//                         copies), the pool's presence chain, the provenance of every pool row, the count prior padded with zeros;
//   air_propose_source:   the provenance of the compacted rows behind air_prune_select on the pool.
// No atomics, no cross-workgroup traffic; every sum has one fixed order: the same bits run to run.
#include <math.h>
#include "scene_device.h"

#define PROPOSE_MAXT 6
#define PROPOSE_THREADS 256

// ============================================================================================================
// residual
// ============================================================================================================
// behind the common head of the carve: the presence row (8 floats), then PROPOSE_THREADS / 64 wave totals
#define PROPOSE_TAIL_FLOATS (8 + PROPOSE_THREADS / 64)
struct ProposeResidualArgs {
    const float *glimpse, *where, *presence, *obs;
    const int *n_in;
    float *res, *res_parts;
    int T, B, NB, RB, H, W, h, w;
    double stepX, stepY;
    float mult, clamp_hi;
    int vec4_glimpse;
};

// One workgroup per (image, row band), air_canvas_unroll_bands' banding, parse_render_kernel's staging: every global operand is
// requested up front, ONE barrier, then each thread walks its pixels (p = tid, tid + nt, ...: a wave's 64 pixels are adjacent) with
// the running canvas in a register, t inner and in order up to n_b -- a workgroup-uniform trip count, no divergence on n_b.  The
// band's sum of res^2: a butterfly inside each wave, the four wave totals through LDS, added in wave order by thread 0.
__global__ __launch_bounds__(PROPOSE_THREADS) void propose_residual_kernel(ProposeResidualArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float smem[];
    const float *__restrict__ glimpse = a.glimpse, *__restrict__ where = a.where, *__restrict__ obs = a.obs;
    float *__restrict__ res = a.res;
    const int T = a.T, B = a.B, RB = a.RB, H = a.H, W = a.W, h = a.h, w = a.w;
    const float mult = a.mult, hi = a.clamp_hi;
    const int HW = H * W, tid = threadIdx.x, nt = PROPOSE_THREADS, lane = tid & 63, wid = tid >> 6;
    const BandCarve c = band_carve(smem, T, RB, W, h, w);
    float *pres = c.tail, *scratch = c.tail + 8;
    const int pitch = w + 2;
    const float inv_W = 1.0f / (float)W;
    const int unit = blockIdx.x;                                   // < B * NB: the grid is exactly the units
    const int b = unit % B, band = unit / B;
    const int r0 = band * RB, r1 = (r0 + RB < H) ? r0 + RB : H, npx = (r1 - r0) * W, pbase = r0 * W;
    const size_t gbase = (size_t)b * HW + pbase;
    const float *ob = obs + gbase;
    const int ob_last = npx - 1;
    // ---- every global load of this unit ----------------------------------------------------------------------------------
    float xo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xo[u] = band_prefetch_obs(ob, ob_last, tid + u * nt);
    band_zero_borders(c, T, h, w, tid, nt);
    band_stage_glimpses(c, glimpse, a.vec4_glimpse != 0, T, B, b, h, w, tid, nt);
    band_axis_tables(c, where, T, B, b, RB, H, W, h, w, r0, r1 - r0, a.stepX, a.stepY, tid, nt);
    if (tid < T) pres[tid] = a.n_in ? (tid < a.n_in[b] ? 1.f : 0.f) : a.presence[(size_t)tid * B + b];
    __syncthreads();
    int nb = 0;                                                    // leading ones: workgroup-uniform
    while (nb < T && pres[nb] > 0.5f) ++nb;
    float s = 0.f;
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
                float acc = 0.f;
                for (int t = 0; t < nb; ++t) {
                    const float2 ex = c.xe[t * W + J], ey = c.ye[t * RB + Ib];
                    const int fx = __float_as_int(ex.x), fy = __float_as_int(ey.x);
                    float v = 0.f;
                    if (fx != ST_INVALID && fy != ST_INVALID)
                        v = bilerp(load_taps_pad(c.glm + (size_t)t * c.hwp, pitch, fy, fx), ex.y, ey.y);
                    acc = acc + v;                                 // (the canvas adds of parse_render_kernel, bit for bit)
                }
                const float d = xo[u] - mult * acc;
                const float r = d > 0.f ? fminf(d, hi) : 0.f;      // a NaN compares false: 0
                res[gbase + p] = r;
                s += r * r;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xo[u] = xn[u];
    }
    if (a.res_parts) {                                             // (uniform)
        const float tot = wave_sum_all(s);
        if (lane == 0) scratch[wid] = tot;
        __syncthreads();
        if (tid == 0) {
            float e = 0.f;
#pragma unroll
            for (int k = 0; k < PROPOSE_THREADS / 64; ++k) e += scratch[k];
            a.res_parts[(size_t)band * B + b] = e;
        }
    }
}

extern "C" int air_propose_residual(const float *glimpse, const float *where, const float *presence, const int *num_objects_in,
                                    const float *obs, float mult, float clamp_hi, int T, int R, int H, int W, int h, int w,
                                    int n_bands, float *res, float *res_parts, void *stream) {
    AIR_REQUIRE(glimpse && where && obs && res && (presence || num_objects_in), AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= PROPOSE_MAXT && R > 0 && H > 0 && W > 0 && h > 0 && w > 0 && n_bands > 0, AIR_E_SHAPE);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(presence) |
                           reinterpret_cast<uintptr_t>(num_objects_in) | reinterpret_cast<uintptr_t>(obs) |
                           reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(res_parts);
    int NB, RB;
    size_t lds;                                                    // (n_bands: the caller sized res_parts for exactly these shares)
    { int st_ = band_launch_prepare(T, R, H, W, h, w, n_bands, where, bits, PROPOSE_TAIL_FLOATS, &NB, &RB, &lds); if (st_) return st_; }
    { int st_ = cv_allow_lds(propose_residual_kernel, lds); if (st_) return st_; }
    const ProposeResidualArgs a = {glimpse, where, presence, obs, num_objects_in, res, res_parts, T, R, NB, RB, H, W, h, w,
                                   lin_step(W), lin_step(H), mult, clamp_hi, (w % 4 == 0) && air_aligned16(glimpse)};
    hipLaunchKernelGGL(propose_residual_kernel, dim3((unsigned)((long)R * NB)), dim3(PROPOSE_THREADS), lds, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// pool
// ============================================================================================================

struct ProposePoolArgs {
    const float *what, *where, *glimpse, *score, *presence;       // the current rows [T, R, .]
    const int *n_in, *source_in;
    const float *p_what, *p_where, *p_glimpse, *p_score;          // the proposal rows: the first P of [>= P, R, .]
    const double *prior;
    int T, P, R, A, G, round, what_vec, glimpse_vec;
    float *pool_what, *pool_where, *pool_glimpse, *pool_score, *pool_presence;
    int *pool_source;
    double *pool_prior;
};

// One wavefront per image: row j < T of the pool from current row j, row T + i from proposal row i; lane j < C writes the presence
// chain and the provenance of pool row j; lane i <= C of image 0 writes the padded prior.
__global__ __launch_bounds__(256) void propose_pool_kernel(ProposePoolArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int T = a.T, P = a.P, R = a.R, A = a.A, G = a.G, C = T + P;
    if (r >= R) return;                                            // wave-uniform
    int n;
    if (a.n_in) {
        n = a.n_in[r];
        n = n < 0 ? 0 : (n > T ? T : n);
    } else {
        const float z = lane < T ? a.presence[(size_t)lane * R + r] : 0.f;
        const unsigned long long present = __ballot(z > 0.5f);     // lanes >= T are clear: ~present is never 0
        n = __ffsll((long long)~present) - 1;
    }
    if (lane < C) {
        const size_t k = (size_t)lane * R + r;
        a.pool_presence[k] = lane < n ? 1.f : 0.f;
        a.pool_source[k] = lane < T ? (a.source_in ? a.source_in[k] : lane) : T + a.round * P + (lane - T);
    }
    if (r == 0 && lane <= C) a.pool_prior[lane] = lane <= T ? a.prior[lane] : 0.0;
    for (int j = 0; j < C; ++j) {                                  // bit copies of all C rows of this image
        const bool cur = j < T;
        const size_t from = (size_t)(cur ? j : j - T) * R + r, to = (size_t)j * R + r;
        const float *wh = cur ? a.where : a.p_where, *sc = cur ? a.score : a.p_score;
        if (lane < 4) reinterpret_cast<unsigned *>(a.pool_where)[to * 4 + lane] = reinterpret_cast<const unsigned *>(wh)[from * 4 + lane];
        if (lane == 4) reinterpret_cast<unsigned *>(a.pool_score)[to] = reinterpret_cast<const unsigned *>(sc)[from];
        copy_row_bits((cur ? a.what : a.p_what) + from * A, a.pool_what + to * A, A, a.what_vec != 0, lane);
        copy_row_bits((cur ? a.glimpse : a.p_glimpse) + from * G, a.pool_glimpse + to * G, G, a.glimpse_vec != 0, lane);
    }
}

extern "C" int air_propose_pool(const float *what, const float *where, const float *glimpse, const float *score, const float *presence,
                                const int *num_objects_in, const int *source_in, const float *prop_what, const float *prop_where,
                                const float *prop_glimpse, const float *prop_score, const double *prior_f64, int round, int T, int P,
                                int R, int A, int G, float *pool_what, float *pool_where, float *pool_glimpse, float *pool_score,
                                float *pool_presence, int *pool_source, double *pool_prior, void *stream) {
    AIR_REQUIRE(what && where && glimpse && score && (presence || num_objects_in) && prop_what && prop_where && prop_glimpse &&
                prop_score && prior_f64 && pool_what && pool_where && pool_glimpse && pool_score && pool_presence && pool_source &&
                pool_prior, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && P > 0 && P <= T && T + P <= PROPOSE_MAXT && R > 0 && A > 0 && G > 0 && round >= 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)T + (long)(round + 1) * P <= (long)INT_MAX, AIR_E_SHAPE);
    const uintptr_t all = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(where) | reinterpret_cast<uintptr_t>(glimpse) |
                          reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(presence) |
                          reinterpret_cast<uintptr_t>(num_objects_in) | reinterpret_cast<uintptr_t>(source_in) |
                          reinterpret_cast<uintptr_t>(prop_what) | reinterpret_cast<uintptr_t>(prop_where) |
                          reinterpret_cast<uintptr_t>(prop_glimpse) | reinterpret_cast<uintptr_t>(prop_score) |
                          reinterpret_cast<uintptr_t>(pool_what) | reinterpret_cast<uintptr_t>(pool_where) |
                          reinterpret_cast<uintptr_t>(pool_glimpse) | reinterpret_cast<uintptr_t>(pool_score) |
                          reinterpret_cast<uintptr_t>(pool_presence) | reinterpret_cast<uintptr_t>(pool_source);
    const uintptr_t dbl = reinterpret_cast<uintptr_t>(prior_f64) | reinterpret_cast<uintptr_t>(pool_prior);
    AIR_REQUIRE((all & 3u) == 0 && (dbl & 7u) == 0, AIR_E_ALIGN);
    const ProposePoolArgs a = {what, where, glimpse, score, presence, num_objects_in, source_in, prop_what, prop_where, prop_glimpse,
                               prop_score, prior_f64, T, P, R, A, G, round,
                               A % 4 == 0 && air_aligned16(what) && air_aligned16(prop_what) && air_aligned16(pool_what),
                               G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(prop_glimpse) && air_aligned16(pool_glimpse),
                               pool_what, pool_where, pool_glimpse, pool_score, pool_presence, pool_source, pool_prior};
    hipLaunchKernelGGL(propose_pool_kernel, dim3(air_cdiv(R, 4)), dim3(256), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// source
// ============================================================================================================
// One wavefront per image; lane j < C composes the provenance of compacted row j.  A kept_step outside 0 .. C-1 (never written by
// air_prune_select) is clipped: no read outside the pool.
__global__ __launch_bounds__(256) void propose_source_kernel(const int *__restrict__ pool_source, const int *__restrict__ kept_step,
                                                             int C, int R, int *__restrict__ source_out) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    if (lane < C) {
        int k = kept_step[(size_t)lane * R + r];
        k = k < 0 ? 0 : (k >= C ? C - 1 : k);
        source_out[(size_t)lane * R + r] = pool_source[(size_t)k * R + r];
    }
}

extern "C" int air_propose_source(const int *pool_source, const int *kept_step, int C, int R, int *source_out, void *stream) {
    AIR_REQUIRE(pool_source && kept_step && source_out, AIR_E_NULL);
    AIR_REQUIRE(C > 0 && C <= PROPOSE_MAXT && R > 0, AIR_E_SHAPE);
    const uintptr_t all = reinterpret_cast<uintptr_t>(pool_source) | reinterpret_cast<uintptr_t>(kept_step) |
                          reinterpret_cast<uintptr_t>(source_out);
    AIR_REQUIRE((all & 3u) == 0, AIR_E_ALIGN);
    hipLaunchKernelGGL(propose_source_kernel, dim3(air_cdiv(R, 4)), dim3(256), 0, air_stream(stream), pool_source, kept_step, C, R,
                       source_out);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
