// Semi-amortised refinement of a scene parse for gfx950: one launch per gradient iteration behind that iteration's decoder / canvas
// forward (and, unless it is the closing call, their backward).
//   air_refine_step: per image the objective J = -rec + log p(what) + log p(where) over the present steps, the keep rule
//                    (the best iterate so far, bit copies of its rows) and one Adam step on the continuous latents.
// One workgroup per image.  No atomics; every sum has one fixed order: the same bits run to run.
#include <math.h>
#include "scene_device.h"
#include "engine_device.h"

#define RF_MAXT 32
#define RF_THREADS 256

struct RfPriors {
    float what_loc, what_scale, scale_loc, scale_scale, shift_loc, shift_scale;   // shift_loc NaN: centred on where_loc
};
struct RfAdam {
    float lr_what, lr_where, beta1, beta2, eps, c1, c2, guard;
};

// m, v and the latent of one element; returns the new latent (before the guard rule)
__device__ __forceinline__ float rf_adam(float z, float d, float mu, float var, float lr, const RfAdam &ad, float &m, float &v) {
    const float g = d + (z - mu) / var;
    m = ad.beta1 * m + (1.f - ad.beta1) * g;
    v = ad.beta2 * v + (1.f - ad.beta2) * (g * g);
    return z - lr * (m / ad.c1) / (sqrtf(v / ad.c2) + ad.eps);
}

// Wave 0 evaluates J in the lane layout of iw_logposterior_kernel (the steps that count are t < n = the number of leading ones of
// the presence chain; their A-wide `what` rows are spread over the lanes as n * A / V vectors, lane t < n takes the four `where`
// components of step t; every lane adds its items in index order, the lanes are added by a butterfly) and decides the keep rule.
// Behind a barrier the four waves copy the rows (if the iterate is taken); behind a second one they update the latents -- the
// copies read what the update overwrites.
template <int V>
__global__ __launch_bounds__(RF_THREADS) void refine_step_kernel(
    float *__restrict__ what, float *__restrict__ where, const float *__restrict__ glimpse, const float *__restrict__ presence,
    const float *__restrict__ rec_parts, int n_bands, const float *__restrict__ dwhat, const float *__restrict__ dwhere,
    const float *__restrict__ where_loc, RfPriors pr, float *__restrict__ m_what, float *__restrict__ v_what,
    float *__restrict__ m_where, float *__restrict__ v_where, RfAdam ad, int iter, int do_update, int T, int B, int A, int G,
    int what_vec, int glimpse_vec, double *__restrict__ best_J, int *__restrict__ best_iter, float *__restrict__ best_what,
    float *__restrict__ best_where, float *__restrict__ best_glimpse, float *__restrict__ J_trace) {
    typedef typename VecOf<V>::type vec_t;
    __shared__ int sh_n, sh_take;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const bool centred = pr.shift_loc != pr.shift_loc;

    if (wave == 0) {
        const float z = lane < T ? presence[(size_t)lane * B + b] : 0.f;
        const unsigned long long present = __ballot(z > 0.5f);     // lanes >= T (T <= 32) are clear: ~present is never 0
        const int n = __ffsll((long long)~present) - 1;

        float s = 0.f;
        const float log_pw = logf(pr.what_scale);
        const int AV = A / V, items = n * AV;
        for (int j = lane; j < items; j += 64) {
            const int t = j / AV, i = j - t * AV;
            const vec_t x = *reinterpret_cast<const vec_t *>(what + ((size_t)t * B + b) * A + (size_t)i * V);
            const float *xf = reinterpret_cast<const float *>(&x);
#pragma unroll
            for (int v = 0; v < V; ++v) s += log_normal(xf[v], pr.what_loc, pr.what_scale, log_pw);
        }
        if (lane < n) {
            const size_t off = ((size_t)lane * B + b) * 4;
            const float4 x = *reinterpret_cast<const float4 *>(where + off);
            float ly = pr.shift_loc, lw = pr.shift_loc;
            if (centred) {
                const float4 l = *reinterpret_cast<const float4 *>(where_loc + off);
                ly = l.y; lw = l.w;
            }
            const float log_ps = logf(pr.scale_scale), log_ph = logf(pr.shift_scale);
            s += log_normal(x.x, pr.scale_loc, pr.scale_scale, log_ps);
            s += log_normal(x.y, ly, pr.shift_scale, log_ph);
            s += log_normal(x.z, pr.scale_loc, pr.scale_scale, log_ps);
            s += log_normal(x.w, lw, pr.shift_scale, log_ph);
        }
        s = wave_sum_all(s);
        float rec = 0.f;                                           // the operations of air_sum_leading
        for (int k = 0; k < n_bands; ++k) rec += rec_parts[(size_t)k * B + b];
        const double J = -(double)rec + (double)s;
        int take = 1;
        if (iter > 0) {
            const double best = best_J[b];
            take = (J == J) && (best != best || J > best) ? 1 : 0;
        }
        if (lane == 0) {
            sh_n = n;
            sh_take = take;
            if (take) {
                best_J[b] = J;
                best_iter[b] = iter;
            }
            if (J_trace) J_trace[(size_t)iter * B + b] = (float)J;
        }
    }
    __syncthreads();
    const int n = sh_n;

    if (sh_take) {                                                 // bit copies of all T rows of this image
        for (int t = wave; t < T; t += RF_THREADS / 64) {
            const size_t row = (size_t)t * B + b;
            if (lane < 4) reinterpret_cast<unsigned *>(best_where)[row * 4 + lane] = reinterpret_cast<const unsigned *>(where)[row * 4 + lane];
            copy_row_bits(what + row * A, best_what + row * A, A, what_vec != 0, lane);
            copy_row_bits(glimpse + row * G, best_glimpse + row * G, G, glimpse_vec != 0, lane);
        }
    }
    if (!do_update) return;                                        // block-uniform
    __syncthreads();

    {                                                              // what: n * A elements over the workgroup
        const float var = pr.what_scale * pr.what_scale;
        for (int j = threadIdx.x; j < n * A; j += RF_THREADS) {
            const int t = j / A, a = j - t * A;
            const size_t o = ((size_t)t * B + b) * A + a;
            float m = m_what[o], v = v_what[o];
            const float z = what[o];
            const float zn = rf_adam(z, dwhat[o], pr.what_loc, var, ad.lr_what, ad, m, v);
            m_what[o] = m;
            v_what[o] = v;
            if (ad.lr_what != 0.f) what[o] = zn;
        }
    }
    if (threadIdx.x < n * 4) {                                     // where: n * 4 <= 128 elements
        const int t = threadIdx.x >> 2, d = threadIdx.x & 3;
        const size_t o = ((size_t)t * B + b) * 4 + d;
        const bool shift = (d & 1) != 0;
        const float sc = shift ? pr.shift_scale : pr.scale_scale;
        float mu = shift ? pr.shift_loc : pr.scale_loc;
        if (shift && centred) mu = where_loc[o];
        float m = m_where[o], v = v_where[o];
        const float z = where[o];
        const float zn = rf_adam(z, dwhere[o], mu, sc * sc, ad.lr_where, ad, m, v);
        m_where[o] = m;
        v_where[o] = v;
        if (ad.lr_where != 0.f) where[o] = guard_where(zn, d, 1, ad.guard);
    }
}

extern "C" int air_refine_step(float *what, float *where, const float *glimpse, const float *presence, const float *rec_parts,
                               int n_bands, const float *dwhat, const float *dwhere, const float *where_loc, float what_p_loc,
                               float what_p_scale, float scale_p_loc, float scale_p_scale, float shift_p_loc, float shift_p_scale,
                               float *m_what, float *v_what, float *m_where, float *v_where, float lr_what, float lr_where,
                               float beta1, float beta2, float eps, float c1, float c2, float guard_eps, int iter, int do_update,
                               int T, int B, int A, int G, double *best_J, int *best_iter, float *best_what, float *best_where,
                               float *best_glimpse, float *J_trace, void *stream) {
    AIR_REQUIRE(what && where && glimpse && presence && rec_parts && best_J && best_iter && best_what && best_where && best_glimpse,
                AIR_E_NULL);
    AIR_REQUIRE(shift_p_loc == shift_p_loc || where_loc, AIR_E_NULL);
    AIR_REQUIRE(!do_update || (dwhat && dwhere && m_what && v_what && m_where && v_where), AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= RF_MAXT && B > 0 && A > 0 && G > 0 && n_bands > 0 && iter >= 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(best_where) && air_aligned16(where_loc) && air_aligned16(dwhere) &&
                air_aligned16(m_where) && air_aligned16(v_where), AIR_E_ALIGN);
    const uintptr_t all = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(presence) |
                          reinterpret_cast<uintptr_t>(rec_parts) | reinterpret_cast<uintptr_t>(dwhat) | reinterpret_cast<uintptr_t>(m_what) |
                          reinterpret_cast<uintptr_t>(v_what) | reinterpret_cast<uintptr_t>(best_iter) | reinterpret_cast<uintptr_t>(best_what) |
                          reinterpret_cast<uintptr_t>(best_glimpse) | reinterpret_cast<uintptr_t>(J_trace);
    AIR_REQUIRE((all & 3u) == 0 && (reinterpret_cast<uintptr_t>(best_J) & 7u) == 0, AIR_E_ALIGN);
    const RfPriors pr = {what_p_loc, what_p_scale, scale_p_loc, scale_p_scale, shift_p_loc, shift_p_scale};
    const RfAdam ad = {lr_what, lr_where, beta1, beta2, eps, c1, c2, guard_eps};
    const int what_vec = A % 4 == 0 && air_aligned16(what) && air_aligned16(best_what);
    const int glimpse_vec = G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(best_glimpse);
    const uintptr_t wbits = reinterpret_cast<uintptr_t>(what);
    const dim3 grid(B), block(RF_THREADS);
#define RF_LAUNCH(V)                                                                                                                \
    hipLaunchKernelGGL(refine_step_kernel<V>, grid, block, 0, air_stream(stream), what, where, glimpse, presence, rec_parts, n_bands, \
                       dwhat, dwhere, where_loc, pr, m_what, v_what, m_where, v_where, ad, iter, do_update, T, B, A, G, what_vec,     \
                       glimpse_vec, best_J, best_iter, best_what, best_where, best_glimpse, J_trace)
    if (A % 4 == 0 && (wbits & 15u) == 0) RF_LAUNCH(4);
    else if (A % 2 == 0 && (wbits & 7u) == 0) RF_LAUNCH(2);
    else RF_LAUNCH(1);
#undef RF_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
