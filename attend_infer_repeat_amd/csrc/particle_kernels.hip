// Best-of-K scene parsing for gfx950: read-outs behind a K-tiled forward pass and its importance weights (iw_kernels.hip).
//   air_iw_logposterior: log q(z | x) of every (image, particle) row;
//   air_particle_select: per image the particle with the largest log w (or log w + log q = log p(x, z)), and bit copies of that
//                        particle's rows into B-row, time-major buffers that air_parse_objects / air_parse_render read;
//   air_particle_spread: per step and image the weighted mean / standard deviation of `where` over the particles that have the step.
// Rows are r = b * K + k: the K particles of an image are adjacent.  No atomics; every sum has one fixed order.
#include <math.h>
#include "scene_device.h"

#define PP_MAXT 32

// log N(x | loc, scale) of a per-element scale: scene_device.h's log_normal with the logarithm taken behind the division.  It stays
// here: with logf(scale) formed at the call site the compiler moves the logarithm in front of the division and the kernel's code changes.
__device__ __forceinline__ float pp_log_normal(float x, float loc, float scale) {
    const float z = (x - loc) / scale;
    return -0.5f * (z * z) - logf(scale) - HALF_LOG_2PI;
}

// One wavefront per row, the lane layout of iw_logweight_kernel: the steps that count are t < n = the number of leading ones
// of the presence chain; their A-wide `what` rows are spread over the lanes as n * A / V vectors of V floats, lane t < n takes
// the four `where` components of step t.  Every lane adds its items in index order, the lanes are added by a butterfly.
template <int V>
__global__ __launch_bounds__(256) void iw_logposterior_kernel(
    const float *__restrict__ what, const float *__restrict__ what_loc, const float *__restrict__ what_scale,
    const float *__restrict__ where, const float *__restrict__ where_loc, const float *__restrict__ where_scale,
    const float *__restrict__ presence, const float *__restrict__ logp, int T, int R, int A, float *__restrict__ log_q) {
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const float z = lane < T ? presence[(size_t)lane * R + r] : 0.f;
    const unsigned long long present = __ballot(z > 0.5f);         // lanes >= T (T <= 32) are clear: ~present is never 0
    const int n = __ffsll((long long)~present) - 1;

    float s = 0.f;
    const int AV = A / V, items = n * AV;
    for (int j = lane; j < items; j += 64) {
        const int t = j / AV, i = j - t * AV;
        const size_t off = ((size_t)t * R + r) * A + (size_t)i * V;
        const vec_t x = *reinterpret_cast<const vec_t *>(what + off);
        const vec_t l = *reinterpret_cast<const vec_t *>(what_loc + off);
        const vec_t c = *reinterpret_cast<const vec_t *>(what_scale + off);
        const float *xf = reinterpret_cast<const float *>(&x), *lf = reinterpret_cast<const float *>(&l),
                    *cf = reinterpret_cast<const float *>(&c);
#pragma unroll
        for (int v = 0; v < V; ++v) s += pp_log_normal(xf[v], lf[v], cf[v]);
    }
    if (lane < n) {
        const size_t off = ((size_t)lane * R + r) * 4;
        const float4 x = *reinterpret_cast<const float4 *>(where + off);
        const float4 l = *reinterpret_cast<const float4 *>(where_loc + off);
        const float4 c = *reinterpret_cast<const float4 *>(where_scale + off);
        s += pp_log_normal(x.x, l.x, c.x);
        s += pp_log_normal(x.y, l.y, c.y);
        s += pp_log_normal(x.z, l.z, c.z);
        s += pp_log_normal(x.w, l.w, c.w);
    }
    s = wave_sum_all(s);
    if (lane == 0) log_q[r] = (float)((double)logp[r] + (double)s);
}

// One wavefront per image; the lanes stride over its K scores (float64, formed from the two fp32 values).  A lane keeps the first
// maximum of its own increasing k; the butterfly prefers the larger score and, between equal scores, the smaller k -- a symmetric
// rule, so every lane ends with the same pair: the SMALLEST k attaining the maximum over the non-NaN scores.  -inf is a value.
__global__ __launch_bounds__(256) void particle_argmax_kernel(const float *__restrict__ log_w, const float *__restrict__ log_q,
                                                              const int *__restrict__ num_steps, int K, int B,
                                                              int *__restrict__ best_particle, float *__restrict__ best_score,
                                                              int *__restrict__ num_objects, int *__restrict__ degenerate) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                            // wave-uniform
    const size_t base = (size_t)b * K;
    double best = 0.0;
    int bk = 0, have = 0;
    for (int k = lane; k < K; k += 64) {
        double s = (double)log_w[base + k];
        if (log_q) s += (double)log_q[base + k];
        if (s == s && (!have || s > best)) { best = s; bk = k; have = 1; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(best, off, 64);
        const int ok = __shfl_xor(bk, off, 64), oh = __shfl_xor(have, off, 64);
        if (oh && (!have || os > best || (os == best && ok < bk))) { best = os; bk = ok; have = 1; }
    }
    if (lane == 0) {
        const int ks = have ? bk : 0;
        best_particle[b] = ks;
        best_score[b] = have ? (float)best : __int_as_float(0x7fc00000);
        num_objects[b] = num_steps[base + ks];
        degenerate[b] = have ? 0 : 1;
    }
}

// One wavefront per (step, image): the selected particle's row t * R + b * K + k* goes to row t * B + b.  Bit copies.
__global__ __launch_bounds__(256) void particle_gather_kernel(const int *__restrict__ best_particle, const float *__restrict__ where,
                                                              const float *__restrict__ what, const float *__restrict__ presence_prob,
                                                              const float *__restrict__ glimpse, int T, int B, int K, int A, int G,
                                                              int what_vec, int glimpse_vec, float *__restrict__ where_sel,
                                                              float *__restrict__ what_sel, float *__restrict__ presence_prob_sel,
                                                              float *__restrict__ glimpse_sel) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);    // t * B + b
    if (row >= (long)T * B) return;                                // wave-uniform
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    const int ks = best_particle[b];
    const size_t src = (size_t)t * B * K + (size_t)b * K + ks, dst = (size_t)row;
    if (lane < 4) reinterpret_cast<unsigned *>(where_sel)[dst * 4 + lane] = reinterpret_cast<const unsigned *>(where)[src * 4 + lane];
    if (lane == 4) reinterpret_cast<unsigned *>(presence_prob_sel)[dst] = reinterpret_cast<const unsigned *>(presence_prob)[src];
    copy_row_bits(what + src * A, what_sel + dst * A, A, what_vec != 0, lane);
    copy_row_bits(glimpse + src * G, glimpse_sel + dst * G, G, glimpse_vec != 0, lane);
}

// One wavefront per image; float64, two passes per step (mean, then the spread about it).  The weights exp(log w - max) are formed
// again in every pass from the cached log-weights: K is small and the kernel is latency-bound.
// A step that exactly one particle of non-zero weight has: (w x) / w is x only to the last float64 place, so the spread about that
// mean would be 1e-16 |x|, not 0 -- the count of such particles decides, and the spread is exactly 0.  A step nobody has: W = 0, mean
// and spread NaN, presence_iw exactly 0.  Non-finite log-weights follow iw_reduce_kernel: an infinite maximum shifts by 0, so all
// -inf or one +inf give NaN means and spreads throughout, one NaN at every step that particle has, and presence_iw has the class of the
// tail sums of the reduce's q_n (NaN; NaN for the steps the +inf particle has and 0 behind them; NaN).
__global__ __launch_bounds__(256) void particle_spread_kernel(const float *__restrict__ log_w, const int *__restrict__ num_steps,
                                                              const float *__restrict__ where, int T, int B, int K,
                                                              float *__restrict__ where_mean, float *__restrict__ where_std,
                                                              float *__restrict__ presence_iw) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                            // wave-uniform
    const size_t base = (size_t)b * K, R = (size_t)B * K;
    const float *lw = log_w + base;
    const int *nk = num_steps + base;
    float mf = -INFINITY;
    for (int k = lane; k < K; k += 64) mf = fmaxf(mf, lw[k]);
    mf = wave_max_all(mf);
    const double m = isinf(mf) ? 0.0 : (double)mf;
    double total = 0.0;
    for (int k = lane; k < K; k += 64) total += exp((double)lw[k] - m);
    total = wave_sum_all(total);
    for (int t = 0; t < T; ++t) {
        double W = 0.0, a[4] = {0.0, 0.0, 0.0, 0.0};
        int cnt = 0;
        for (int k = lane; k < K; k += 64) {
            if (nk[k] > t) {
                const double w = exp((double)lw[k] - m);
                const float4 x = *reinterpret_cast<const float4 *>(where + ((size_t)t * R + base + k) * 4);
                cnt += w > 0.0 ? 1 : 0;
                W += w;
                a[0] += w * (double)x.x; a[1] += w * (double)x.y; a[2] += w * (double)x.z; a[3] += w * (double)x.w;
            }
        }
        W = wave_sum_all(W);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        double mean[4], v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) mean[j] = wave_sum_all(a[j]) / W;
        for (int k = lane; k < K; k += 64) {
            if (nk[k] > t) {
                const double w = exp((double)lw[k] - m);
                const float4 x = *reinterpret_cast<const float4 *>(where + ((size_t)t * R + base + k) * 4);
                const double d0 = (double)x.x - mean[0], d1 = (double)x.y - mean[1], d2 = (double)x.z - mean[2],
                             d3 = (double)x.w - mean[3];
                v[0] += w * (d0 * d0); v[1] += w * (d1 * d1); v[2] += w * (d2 * d2); v[3] += w * (d3 * d3);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double q = wave_sum_all(v[j]) / W;
            v[j] = (cnt == 1 && q == q) ? 0.0 : sqrt(q < 0.0 ? 0.0 : q);   // (a NaN stays a NaN: W == 0, or a weight of +inf)
        }
        if (lane == 0) {
            const size_t o = (size_t)t * B + b;
            *reinterpret_cast<float4 *>(where_mean + o * 4) = make_float4((float)mean[0], (float)mean[1], (float)mean[2], (float)mean[3]);
            *reinterpret_cast<float4 *>(where_std + o * 4) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
            presence_iw[o] = (float)(W / total);
        }
    }
}

extern "C" int air_iw_logposterior(const float *what, const float *what_loc, const float *what_scale, const float *where,
                                   const float *where_loc, const float *where_scale, const float *presence, const float *logp,
                                   int T, int R, int K, int A, float *log_q, void *stream) {
    AIR_REQUIRE(what && what_loc && what_scale && where && where_loc && where_scale && presence && logp && log_q, AIR_E_NULL);
    AIR_REQUIRE(K > 0 && T > 0 && T <= PP_MAXT && R > 0 && A > 0 && R % K == 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_loc) && air_aligned16(where_scale), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(what_loc) |
                           reinterpret_cast<uintptr_t>(what_scale);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const dim3 grid(air_cdiv(R, 4)), block(256);
#define PP_LAUNCH(V)                                                                                                              \
    hipLaunchKernelGGL(iw_logposterior_kernel<V>, grid, block, 0, air_stream(stream), what, what_loc, what_scale, where, where_loc, \
                       where_scale, presence, logp, T, R, A, log_q)
    if (A % 4 == 0 && (bits & 15u) == 0) PP_LAUNCH(4);
    else if (A % 2 == 0 && (bits & 7u) == 0) PP_LAUNCH(2);
    else PP_LAUNCH(1);
#undef PP_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_particle_select(const float *log_w, const float *log_q, const int *num_steps, const float *where, const float *what,
                                   const float *presence_prob, const float *glimpse, int T, int R, int K, int A, int G, int criterion,
                                   int *best_particle, float *best_score, int *num_objects, int *degenerate, float *where_sel,
                                   float *what_sel, float *presence_prob_sel, float *glimpse_sel, void *stream) {
    AIR_REQUIRE(log_w && num_steps && where && what && presence_prob && glimpse && best_particle && best_score && num_objects &&
                degenerate && where_sel && what_sel && presence_prob_sel && glimpse_sel, AIR_E_NULL);
    AIR_REQUIRE(criterion == 0 || criterion == 1, AIR_E_SHAPE);
    AIR_REQUIRE(criterion == 0 || log_q, AIR_E_NULL);
    AIR_REQUIRE(K > 0 && T > 0 && T <= PP_MAXT && R > 0 && A > 0 && G > 0 && R % K == 0, AIR_E_SHAPE);
    const uintptr_t all = reinterpret_cast<uintptr_t>(where) | reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(glimpse) |
                          reinterpret_cast<uintptr_t>(where_sel) | reinterpret_cast<uintptr_t>(what_sel) |
                          reinterpret_cast<uintptr_t>(glimpse_sel) | reinterpret_cast<uintptr_t>(presence_prob) |
                          reinterpret_cast<uintptr_t>(presence_prob_sel);
    AIR_REQUIRE((all & 3u) == 0, AIR_E_ALIGN);
    const int B = R / K;
    const int what_vec = A % 4 == 0 && air_aligned16(what) && air_aligned16(what_sel);
    const int glimpse_vec = G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(glimpse_sel);
    hipLaunchKernelGGL(particle_argmax_kernel, dim3(air_cdiv(B, 4)), dim3(256), 0, air_stream(stream), log_w,
                       criterion == 1 ? log_q : (const float *)nullptr, num_steps, K, B, best_particle, best_score, num_objects,
                       degenerate);
    AIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(particle_gather_kernel, dim3(air_cdiv((long)T * B, 4)), dim3(256), 0, air_stream(stream), best_particle, where,
                       what, presence_prob, glimpse, T, B, K, A, G, what_vec, glimpse_vec, where_sel, what_sel, presence_prob_sel,
                       glimpse_sel);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_particle_spread(const float *log_w, const int *num_steps, const float *where, int T, int R, int K,
                                   float *where_mean, float *where_std, float *presence_iw, void *stream) {
    AIR_REQUIRE(log_w && num_steps && where && where_mean && where_std && presence_iw, AIR_E_NULL);
    AIR_REQUIRE(K > 0 && T > 0 && T <= PP_MAXT && R > 0 && R % K == 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_mean) && air_aligned16(where_std), AIR_E_ALIGN);
    const int B = R / K;
    hipLaunchKernelGGL(particle_spread_kernel, dim3(air_cdiv(B, 4)), dim3(256), 0, air_stream(stream), log_w, num_steps, where, T, B, K,
                       where_mean, where_std, presence_iw);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
