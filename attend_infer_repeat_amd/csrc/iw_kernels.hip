// K-particle importance-weighted evaluation of AIR for gfx950 (no backward: a read-out of the forward's buffers).
//   air_iw_logweight: log w = log p(x, z) - log q(z | x) of every (image, particle) row of a K-tiled forward pass;
//   air_iw_reduce:    per image, over its K particles: the importance-weighted bound, the plain ELBO of the same particles, the
//                     effective sample size and the self-normalised posterior over the object count (+ float64 running totals).
// Rows are r = b * K + k: the K particles of an image are adjacent.
#include "iw_device.h"

// One wavefront per row.  The chain of presences is monotone, so the steps that count are t < n = the number of leading
// ones; their A-wide `what` rows are spread over the lanes as n * A / V vectors of V floats (V = 4 / 2 / 1: what the row
// starts allow), lane t < n takes the four `where` components of step t.  Every lane adds its items in index order, the
// lanes are added by a butterfly: one fixed order, the same bits run to run.
template <int V>
__global__ __launch_bounds__(256) void iw_logweight_kernel(
    const float *__restrict__ what, const float *__restrict__ what_loc, const float *__restrict__ what_scale,
    const float *__restrict__ where, const float *__restrict__ where_loc, const float *__restrict__ where_scale,
    const float *__restrict__ presence, const float *__restrict__ rec, const float *__restrict__ logp,
    const double *__restrict__ prior, int T, int R, int A, IwPriors pr, int normalize, float *__restrict__ logw,
    int *__restrict__ n_out) {
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const float z = lane < T ? presence[(size_t)lane * R + r] : 0.f;
    const unsigned long long present = __ballot(z > 0.5f);         // lanes >= T (T <= 32) are clear: ~present is never 0
    const int n = __ffsll((long long)~present) - 1;

    float s = 0.f;
    const float log_pw = logf(pr.what_scale);
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
        for (int v = 0; v < V; ++v) s += iw_log_ratio(xf[v], lf[v], cf[v], pr.what_loc, pr.what_scale, log_pw);
    }
    if (lane < n) {
        const size_t off = ((size_t)lane * R + r) * 4;
        const float4 x = *reinterpret_cast<const float4 *>(where + off);
        const float4 l = *reinterpret_cast<const float4 *>(where_loc + off);
        const float4 c = *reinterpret_cast<const float4 *>(where_scale + off);
        const float log_ps = logf(pr.scale_scale), log_ph = logf(pr.shift_scale);
        const bool centred = pr.shift_loc != pr.shift_loc;
        s += iw_log_ratio(x.x, l.x, c.x, pr.scale_loc, pr.scale_scale, log_ps);
        s += iw_log_ratio(x.y, l.y, c.y, centred ? l.y : pr.shift_loc, pr.shift_scale, log_ph);
        s += iw_log_ratio(x.z, l.z, c.z, pr.scale_loc, pr.scale_scale, log_ps);
        s += iw_log_ratio(x.w, l.w, c.w, centred ? l.w : pr.shift_loc, pr.shift_scale, log_ph);
    }
    s = wave_sum_all(s);

    // log pi(n) in float64 like the rest of the num-steps math; the table is not normalised in the training loss
    double total = 1.0;
    if (normalize) {
        total = 0.0;
        for (int i = 0; i <= T; ++i) total += prior[i];
    }
    const double log_prior = log(prior[n] / total);
    const double lw = -(double)rec[r] + (log_prior - (double)logp[r]) + (double)s;
    if (lane == 0) {
        logw[r] = (float)lw;
        n_out[r] = n;
    }
}

// One wavefront per image over its K log-weights (K arbitrary: the lanes stride over them, passes re-read them from cache).
__global__ __launch_bounds__(256) void iw_reduce_kernel(const float *__restrict__ logw, const int *__restrict__ n, int K, int B,
                                                        int T, float *__restrict__ iw_bound, float *__restrict__ elbo,
                                                        float *__restrict__ ess, float *__restrict__ q_n) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                            // wave-uniform
    const float *lw = logw + (size_t)b * K;
    const int *nk = n + (size_t)b * K;
    float m = -INFINITY, sum = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float v = lw[k];
        m = fmaxf(m, v);
        sum += v;
    }
    m = wave_max_all(m);
    sum = wave_sum_all(sum);
    const float shift = isinf(m) ? 0.f : m;                        // (all weights zero / one infinite: the usual logsumexp convention)
    float s1 = 0.f, s2 = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = expf(lw[k] - shift);
        s1 += w;
        s2 += w * w;
    }
    s1 = wave_sum_all(s1);
    s2 = wave_sum_all(s2);
    for (int c = 0; c <= T; ++c) {
        float sc = 0.f;
        for (int k = lane; k < K; k += 64) sc += nk[k] == c ? expf(lw[k] - shift) : 0.f;
        sc = wave_sum_all(sc);
        if (lane == 0) q_n[(size_t)b * (T + 1) + c] = sc / s1;
    }
    if (lane == 0) {
        iw_bound[b] = shift + logf(s1) - logf((float)K);
        elbo[b] = sum / (float)K;
        ess[b] = s1 * s1 / s2;
    }
}

// Running totals over evaluation calls: ONE workgroup adds this call's B images in a fixed order in float64 (thread i takes images
// i, i + 256, ...; a fixed tree over the threads) and adds the result to acc[0..4] = {sum iw_bound, sum elbo, sum ess, number of
// images whose argmax q_n equals gt_steps, number of images}.  No atomics.
__global__ __launch_bounds__(256) void iw_accumulate_kernel(const float *__restrict__ iw_bound, const float *__restrict__ elbo,
                                                            const float *__restrict__ ess, const float *__restrict__ q_n,
                                                            const int *__restrict__ gt, int B, int T, double *__restrict__ acc) {
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < B; b += 256) {
        a[0] += (double)iw_bound[b];
        a[1] += (double)elbo[b];
        a[2] += (double)ess[b];
        if (gt) {
            const float *q = q_n + (size_t)b * (T + 1);
            int best = 0;
            float qbest = q[0];
            for (int c = 1; c <= T; ++c)
                if (q[c] > qbest) { qbest = q[c]; best = c; }
            a[3] += best == gt[b] ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sh[i][tid] = a[i];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sh[i][tid] += sh[i][tid + half];
        }
        __syncthreads();
    }
    if (tid < 4) acc[tid] += sh[tid][0];
    if (tid == 4) acc[4] += (double)B;
}

extern "C" int air_iw_logweight(const float *what, const float *what_loc, const float *what_scale, const float *where,
                                const float *where_loc, const float *where_scale, const float *presence, const float *rec,
                                const float *logp, const double *prior_f64, int T, int R, int K, int A, float what_p_loc,
                                float what_p_scale, float scale_p_loc, float scale_p_scale, float shift_p_loc,
                                float shift_p_scale, int normalize_prior, float *logw, int *num_steps, void *stream) {
    AIR_REQUIRE(what && what_loc && what_scale && where && where_loc && where_scale && presence && rec && logp && prior_f64 &&
                logw && num_steps, AIR_E_NULL);
    AIR_REQUIRE(K > 0 && T > 0 && T <= IW_MAXT && R > 0 && A > 0 && R % K == 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_loc) && air_aligned16(where_scale), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(what_loc) |
                           reinterpret_cast<uintptr_t>(what_scale);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const IwPriors pr = {what_p_loc, what_p_scale, scale_p_loc, scale_p_scale, shift_p_loc, shift_p_scale};
    const dim3 grid(air_cdiv(R, 4)), block(256);
#define IW_LAUNCH(V)                                                                                                           \
    hipLaunchKernelGGL(iw_logweight_kernel<V>, grid, block, 0, air_stream(stream), what, what_loc, what_scale, where, where_loc, \
                       where_scale, presence, rec, logp, prior_f64, T, R, A, pr, normalize_prior, logw, num_steps)
    if (A % 4 == 0 && (bits & 15u) == 0) IW_LAUNCH(4);
    else if (A % 2 == 0 && (bits & 7u) == 0) IW_LAUNCH(2);
    else IW_LAUNCH(1);
#undef IW_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_iw_reduce(const float *logw, const int *num_steps, int T, int R, int K, float *iw_bound, float *elbo,
                             float *ess, float *q_n_iw, const int *gt_steps, double *acc, void *stream) {
    AIR_REQUIRE(logw && num_steps && iw_bound && elbo && ess && q_n_iw, AIR_E_NULL);
    AIR_REQUIRE(!gt_steps || acc, AIR_E_NULL);
    AIR_REQUIRE(K > 0 && T > 0 && T <= IW_MAXT && R > 0 && R % K == 0, AIR_E_SHAPE);
    const int B = R / K;
    hipLaunchKernelGGL(iw_reduce_kernel, dim3(air_cdiv(B, 4)), dim3(256), 0, air_stream(stream), logw, num_steps, K, B, T,
                       iw_bound, elbo, ess, q_n_iw);
    AIR_LAUNCH_CHECK();
    if (acc) {
        hipLaunchKernelGGL(iw_accumulate_kernel, dim3(1), dim3(256), 0, air_stream(stream), iw_bound, elbo, ess, q_n_iw, gt_steps,
                           B, T, acc);
        AIR_LAUNCH_CHECK();
    }
    return AIR_OK;
}
