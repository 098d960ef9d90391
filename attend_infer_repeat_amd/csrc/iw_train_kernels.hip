// Training on the K-particle importance-weighted bound for gfx950: the backward side of iw_kernels.hip.
//   air_iw_logweight_bwd: the gradient of air_iw_logweight's row value log w[r] given an upstream g[r];
//   air_iw_vimco:         per image, over its K adjacent log-weights: the bound, the self-normalised weights (the coefficients of
//                         grad log w) and VIMCO's leave-one-out learning signal (the coefficients of grad log q(n)), float64 inside;
//   air_iw_logposterior_bwd: the gradient of air_iw_logposterior's row value log q[r] given an upstream g[r] (the wake-phase update of
//                         reweighted wake-sleep: the samples are fixed values, their gradients optional).
// Rows are r = b * K + k: the K particles of an image are adjacent.
#include <limits.h>
#include "iw_device.h"

// One wavefront per row, the lane layout of iw_logweight_kernel: n = the number of leading ones of the presence chain, the A-wide rows
// of all T steps spread over the lanes as T * A / V vectors of V floats, lane t < T takes the four `where` components of step t.  Rows
// of steps t >= n are written as exact zeros.  Every output element is a function of one item and g[r]; with
//     zq = (x - loc) / scale,  zp = (x - p_loc) / p_scale,  a = zq / scale,  b = zp / p_scale
// it is, in this order and without contraction,
//     d x     = g * (a - b)
//     d loc   = g * (0 - a)            (a shift prior centred on where_loc: g * (b - a), the prior term moves with where_loc)
//     d scale = g * ((1 - zq * zq) / scale)
// No clamps: a zero scale gives the inf / NaN of the plain formula in that row only.
struct IwGrad3 { float x, loc, scale; };
__device__ __forceinline__ IwGrad3 iw_log_ratio_grad(float x, float loc, float scale, float p_loc, float p_scale, bool centred, float g) {
#pragma clang fp contract(off)
    const float zq = (x - loc) / scale, zp = (x - p_loc) / p_scale;
    const float a = zq / scale, b = zp / p_scale;
    IwGrad3 d;
    d.x = g * (a - b);
    d.loc = g * ((centred ? b : 0.f) - a);
    d.scale = g * ((1.f - zq * zq) / scale);
    return d;
}

template <int V>
__global__ __launch_bounds__(256) void iw_logweight_bwd_kernel(
    const float *__restrict__ what, const float *__restrict__ what_loc, const float *__restrict__ what_scale,
    const float *__restrict__ where, const float *__restrict__ where_loc, const float *__restrict__ where_scale,
    const float *__restrict__ presence, const float *__restrict__ g, int T, int R, int A, IwPriors pr,
    float *__restrict__ d_what, float *__restrict__ d_what_loc, float *__restrict__ d_what_scale, float *__restrict__ d_where,
    float *__restrict__ d_where_loc, float *__restrict__ d_where_scale, float *__restrict__ d_rec, float *__restrict__ d_logp) {
#pragma clang fp contract(off)
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const float z = lane < T ? presence[(size_t)lane * R + r] : 0.f;
    const unsigned long long present = __ballot(z > 0.5f);         // lanes >= T (T <= 32) are clear: ~present is never 0
    const int n = __ffsll((long long)~present) - 1;
    const float gr = g[r];

    const int AV = A / V, items = T * AV;
    for (int j = lane; j < items; j += 64) {
        const int t = j / AV, i = j - t * AV;
        const size_t off = ((size_t)t * R + r) * A + (size_t)i * V;
        vec_t dx, dl, dc;
        float *dxf = reinterpret_cast<float *>(&dx), *dlf = reinterpret_cast<float *>(&dl), *dcf = reinterpret_cast<float *>(&dc);
        if (t < n) {
            const vec_t x = *reinterpret_cast<const vec_t *>(what + off);
            const vec_t l = *reinterpret_cast<const vec_t *>(what_loc + off);
            const vec_t c = *reinterpret_cast<const vec_t *>(what_scale + off);
            const float *xf = reinterpret_cast<const float *>(&x), *lf = reinterpret_cast<const float *>(&l),
                        *cf = reinterpret_cast<const float *>(&c);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const IwGrad3 d = iw_log_ratio_grad(xf[v], lf[v], cf[v], pr.what_loc, pr.what_scale, false, gr);
                dxf[v] = d.x; dlf[v] = d.loc; dcf[v] = d.scale;
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) dxf[v] = dlf[v] = dcf[v] = 0.f;
        }
        *reinterpret_cast<vec_t *>(d_what + off) = dx;
        *reinterpret_cast<vec_t *>(d_what_loc + off) = dl;
        *reinterpret_cast<vec_t *>(d_what_scale + off) = dc;
    }
    if (lane < T) {
        const size_t off = ((size_t)lane * R + r) * 4;
        float4 dx = make_float4(0.f, 0.f, 0.f, 0.f), dl = dx, dc = dx;
        if (lane < n) {
            const float4 x = *reinterpret_cast<const float4 *>(where + off);
            const float4 l = *reinterpret_cast<const float4 *>(where_loc + off);
            const float4 c = *reinterpret_cast<const float4 *>(where_scale + off);
            const bool centred = pr.shift_loc != pr.shift_loc;
            const IwGrad3 d0 = iw_log_ratio_grad(x.x, l.x, c.x, pr.scale_loc, pr.scale_scale, false, gr);
            const IwGrad3 d1 = iw_log_ratio_grad(x.y, l.y, c.y, centred ? l.y : pr.shift_loc, pr.shift_scale, centred, gr);
            const IwGrad3 d2 = iw_log_ratio_grad(x.z, l.z, c.z, pr.scale_loc, pr.scale_scale, false, gr);
            const IwGrad3 d3 = iw_log_ratio_grad(x.w, l.w, c.w, centred ? l.w : pr.shift_loc, pr.shift_scale, centred, gr);
            dx = make_float4(d0.x, d1.x, d2.x, d3.x);
            dl = make_float4(d0.loc, d1.loc, d2.loc, d3.loc);
            dc = make_float4(d0.scale, d1.scale, d2.scale, d3.scale);
        }
        *reinterpret_cast<float4 *>(d_where + off) = dx;
        *reinterpret_cast<float4 *>(d_where_loc + off) = dl;
        *reinterpret_cast<float4 *>(d_where_scale + off) = dc;
    }
    if (lane == 0) {
        d_rec[r] = -gr;
        d_logp[r] = -gr;
    }
}

// The gradient of air_iw_logposterior's row value log q[r] = logp[r] + sum_{t<n} sum log N(x | loc, scale) given an upstream g[r]: the
// layout above without the prior terms.  Per element, with zq = (x - loc) / scale and a = zq / scale, in this order and without
// contraction,
//     d loc   = g * a
//     d scale = g * ((zq * zq - 1) / scale)
//     d x     = g * (0 - a)
// d_what / d_where may be NULL (the reweighted wake-sleep update holds the samples fixed and has no use for them): not written then.
struct IwPostGrad3 { float x, loc, scale; };
__device__ __forceinline__ IwPostGrad3 iw_log_normal_grad(float x, float loc, float scale, float g) {
#pragma clang fp contract(off)
    const float zq = (x - loc) / scale;
    const float a = zq / scale;
    IwPostGrad3 d;
    d.loc = g * a;
    d.scale = g * ((zq * zq - 1.f) / scale);
    d.x = g * (0.f - a);
    return d;
}

template <int V>
__global__ __launch_bounds__(256) void iw_logposterior_bwd_kernel(
    const float *__restrict__ what, const float *__restrict__ what_loc, const float *__restrict__ what_scale,
    const float *__restrict__ where, const float *__restrict__ where_loc, const float *__restrict__ where_scale,
    const float *__restrict__ presence, const float *__restrict__ g, int T, int R, int A, float *__restrict__ d_what,
    float *__restrict__ d_what_loc, float *__restrict__ d_what_scale, float *__restrict__ d_where, float *__restrict__ d_where_loc,
    float *__restrict__ d_where_scale, float *__restrict__ d_logp) {
#pragma clang fp contract(off)
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const float z = lane < T ? presence[(size_t)lane * R + r] : 0.f;
    const unsigned long long present = __ballot(z > 0.5f);         // lanes >= T (T <= 32) are clear: ~present is never 0
    const int n = __ffsll((long long)~present) - 1;
    const float gr = g[r];

    const int AV = A / V, items = T * AV;
    for (int j = lane; j < items; j += 64) {
        const int t = j / AV, i = j - t * AV;
        const size_t off = ((size_t)t * R + r) * A + (size_t)i * V;
        vec_t dx, dl, dc;
        float *dxf = reinterpret_cast<float *>(&dx), *dlf = reinterpret_cast<float *>(&dl), *dcf = reinterpret_cast<float *>(&dc);
        if (t < n) {
            const vec_t x = *reinterpret_cast<const vec_t *>(what + off);
            const vec_t l = *reinterpret_cast<const vec_t *>(what_loc + off);
            const vec_t c = *reinterpret_cast<const vec_t *>(what_scale + off);
            const float *xf = reinterpret_cast<const float *>(&x), *lf = reinterpret_cast<const float *>(&l),
                        *cf = reinterpret_cast<const float *>(&c);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const IwPostGrad3 d = iw_log_normal_grad(xf[v], lf[v], cf[v], gr);
                dxf[v] = d.x; dlf[v] = d.loc; dcf[v] = d.scale;
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) dxf[v] = dlf[v] = dcf[v] = 0.f;
        }
        if (d_what) *reinterpret_cast<vec_t *>(d_what + off) = dx;     // uniform over the launch
        *reinterpret_cast<vec_t *>(d_what_loc + off) = dl;
        *reinterpret_cast<vec_t *>(d_what_scale + off) = dc;
    }
    if (lane < T) {
        const size_t off = ((size_t)lane * R + r) * 4;
        float4 dx = make_float4(0.f, 0.f, 0.f, 0.f), dl = dx, dc = dx;
        if (lane < n) {
            const float4 x = *reinterpret_cast<const float4 *>(where + off);
            const float4 l = *reinterpret_cast<const float4 *>(where_loc + off);
            const float4 c = *reinterpret_cast<const float4 *>(where_scale + off);
            const IwPostGrad3 d0 = iw_log_normal_grad(x.x, l.x, c.x, gr);
            const IwPostGrad3 d1 = iw_log_normal_grad(x.y, l.y, c.y, gr);
            const IwPostGrad3 d2 = iw_log_normal_grad(x.z, l.z, c.z, gr);
            const IwPostGrad3 d3 = iw_log_normal_grad(x.w, l.w, c.w, gr);
            dx = make_float4(d0.x, d1.x, d2.x, d3.x);
            dl = make_float4(d0.loc, d1.loc, d2.loc, d3.loc);
            dc = make_float4(d0.scale, d1.scale, d2.scale, d3.scale);
        }
        if (d_where) *reinterpret_cast<float4 *>(d_where + off) = dx;
        *reinterpret_cast<float4 *>(d_where_loc + off) = dl;
        *reinterpret_cast<float4 *>(d_where_scale + off) = dc;
    }
    if (lane == 0) d_logp[r] = gr;
}

__device__ __forceinline__ double wave_max_all_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_min_all_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_all_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wavefront per image over its K log-weights lw_k (K >= 2 arbitrary: the lanes stride over them, the passes re-read them from
// cache).  All arithmetic in float64, every output rounded once to float32.  With m = max_k lw_k, k* the lowest index that attains
// it, e_k = exp(lw_k - m) (e_k* = 1 exactly), E = sum_{j != k*} e_j and S = 1 + E:
//     bound    = m + log S - log K                      ess = S * S / sum_k e_k^2
//     wnorm_k  = e_k / S
//     loo_k    = sum_{j != k} e_j = E for k = k*, 1 + (E - e_k) otherwise          (never a difference of two nearly equal sums)
//     lgeo_k   = (1 / (K - 1)) sum_{j != k} lw_j: -inf when another particle is at -inf, else (L - lw_k) / (K - 1) with L the sum of
//                the finite log-weights (lw_k left out of the subtraction when it is -inf itself)
//     signal_k = log S - log(loo_k + exp(lgeo_k - m))   (= bound - bound without k, the shift m cancelled by hand)
// Every lane adds its items in index order, the lanes are added by a butterfly: one fixed order, no atomics, one writer per element.
// DEGENERATE image: a NaN or +inf log-weight, or all at -inf -> wnorm and signal rows exact zeros, bound = ess = 0, degenerate = 1.
__global__ __launch_bounds__(256) void iw_vimco_kernel(const float *__restrict__ logw, int K, int B, float *__restrict__ bound,
                                                       float *__restrict__ wnorm, float *__restrict__ signal, float *__restrict__ ess,
                                                       int *__restrict__ degenerate) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                            // wave-uniform
    const float *lw = logw + (size_t)b * K;
    float *wn = wnorm + (size_t)b * K, *sg = signal + (size_t)b * K;

    double m = -INFINITY;
    int kmax = INT_MAX, bad = 0;
    for (int k = lane; k < K; k += 64) {
        const double v = (double)lw[k];
        bad |= (v != v || v == INFINITY) ? 1 : 0;
        if (v > m) { m = v; kmax = k; }                            // strictly greater: the lowest index of the lane's stride
    }
    const double m_all = wave_max_all_f64(m);
    kmax = wave_min_all_i32(m == m_all ? kmax : INT_MAX);
    const bool degen = __ballot(bad != 0) != 0ull || m_all == -INFINITY;
    if (degen) {                                                   // wave-uniform
        for (int k = lane; k < K; k += 64) { wn[k] = 0.f; sg[k] = 0.f; }
        if (lane == 0) { bound[b] = 0.f; ess[b] = 0.f; degenerate[b] = 1; }
        return;
    }

    double E = 0.0, s2 = 0.0, L = 0.0;
    int ninf = 0;
    for (int k = lane; k < K; k += 64) {
        const double v = (double)lw[k];
        const double e = exp(v - m_all);
        if (k != kmax) E += e;
        s2 += e * e;
        if (v == -INFINITY) ninf += 1;
        else L += v;
    }
    E = wave_sum_all(E);
    s2 = wave_sum_all(s2);
    L = wave_sum_all(L);
    ninf = wave_sum_all_i32(ninf);
    const double S = 1.0 + E, logS = log(S);
    for (int k = lane; k < K; k += 64) {
        const double v = (double)lw[k];
        const double e = exp(v - m_all);
        const bool own_inf = v == -INFINITY;
        const double loo = k == kmax ? E : 1.0 + (E - e);
        const double lgeo = (ninf - (own_inf ? 1 : 0)) > 0 ? -INFINITY : (L - (own_inf ? 0.0 : v)) / (double)(K - 1);
        wn[k] = (float)(e / S);
        sg[k] = (float)(logS - log(loo + exp(lgeo - m_all)));
    }
    if (lane == 0) {
        bound[b] = (float)(m_all + logS - log((double)K));
        ess[b] = (float)(S * S / s2);
        degenerate[b] = 0;
    }
}

extern "C" int air_iw_logweight_bwd(const float *what, const float *what_loc, const float *what_scale, const float *where,
                                    const float *where_loc, const float *where_scale, const float *presence, const float *g, int T,
                                    int R, int K, int A, float what_p_loc, float what_p_scale, float scale_p_loc, float scale_p_scale,
                                    float shift_p_loc, float shift_p_scale, float *d_what, float *d_what_loc, float *d_what_scale,
                                    float *d_where, float *d_where_loc, float *d_where_scale, float *d_rec, float *d_logp,
                                    void *stream) {
    AIR_REQUIRE(what && what_loc && what_scale && where && where_loc && where_scale && presence && g && d_what && d_what_loc &&
                d_what_scale && d_where && d_where_loc && d_where_scale && d_rec && d_logp, AIR_E_NULL);
    AIR_REQUIRE(K > 0 && T > 0 && T <= IW_MAXT && R > 0 && A > 0 && R % K == 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)T * R * A <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_loc) && air_aligned16(where_scale) && air_aligned16(d_where) &&
                air_aligned16(d_where_loc) && air_aligned16(d_where_scale), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(what_loc) |
                           reinterpret_cast<uintptr_t>(what_scale) | reinterpret_cast<uintptr_t>(d_what) |
                           reinterpret_cast<uintptr_t>(d_what_loc) | reinterpret_cast<uintptr_t>(d_what_scale);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const IwPriors pr = {what_p_loc, what_p_scale, scale_p_loc, scale_p_scale, shift_p_loc, shift_p_scale};
    const dim3 grid(air_cdiv(R, 4)), block(256);
#define IW_BWD_LAUNCH(V)                                                                                                          \
    hipLaunchKernelGGL(iw_logweight_bwd_kernel<V>, grid, block, 0, air_stream(stream), what, what_loc, what_scale, where, where_loc, \
                       where_scale, presence, g, T, R, A, pr, d_what, d_what_loc, d_what_scale, d_where, d_where_loc, d_where_scale, \
                       d_rec, d_logp)
    if (A % 4 == 0 && (bits & 15u) == 0) IW_BWD_LAUNCH(4);
    else if (A % 2 == 0 && (bits & 7u) == 0) IW_BWD_LAUNCH(2);
    else IW_BWD_LAUNCH(1);
#undef IW_BWD_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_iw_logposterior_bwd(const float *what, const float *what_loc, const float *what_scale, const float *where,
                                       const float *where_loc, const float *where_scale, const float *presence, const float *g, int T,
                                       int R, int K, int A, float *d_what, float *d_what_loc, float *d_what_scale, float *d_where,
                                       float *d_where_loc, float *d_where_scale, float *d_logp, void *stream) {
    AIR_REQUIRE(what && what_loc && what_scale && where && where_loc && where_scale && presence && g && d_what_loc && d_what_scale &&
                d_where_loc && d_where_scale && d_logp, AIR_E_NULL);                 // d_what / d_where: optional
    AIR_REQUIRE(K > 0 && T > 0 && T <= IW_MAXT && R > 0 && A > 0 && R % K == 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)T * R * A <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_loc) && air_aligned16(where_scale) && air_aligned16(d_where) &&
                air_aligned16(d_where_loc) && air_aligned16(d_where_scale), AIR_E_ALIGN);   // (a NULL d_where is aligned)
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(what_loc) |
                           reinterpret_cast<uintptr_t>(what_scale) | reinterpret_cast<uintptr_t>(d_what) |
                           reinterpret_cast<uintptr_t>(d_what_loc) | reinterpret_cast<uintptr_t>(d_what_scale);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const dim3 grid(air_cdiv(R, 4)), block(256);
#define IW_POST_BWD_LAUNCH(V)                                                                                                      \
    hipLaunchKernelGGL(iw_logposterior_bwd_kernel<V>, grid, block, 0, air_stream(stream), what, what_loc, what_scale, where,        \
                       where_loc, where_scale, presence, g, T, R, A, d_what, d_what_loc, d_what_scale, d_where, d_where_loc,       \
                       d_where_scale, d_logp)
    if (A % 4 == 0 && (bits & 15u) == 0) IW_POST_BWD_LAUNCH(4);
    else if (A % 2 == 0 && (bits & 7u) == 0) IW_POST_BWD_LAUNCH(2);
    else IW_POST_BWD_LAUNCH(1);
#undef IW_POST_BWD_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_iw_vimco(const float *logw, int R, int K, float *bound, float *wnorm, float *signal, float *ess, int *degenerate,
                            void *stream) {
    AIR_REQUIRE(logw && bound && wnorm && signal && ess && degenerate, AIR_E_NULL);
    AIR_REQUIRE(K >= 2 && R > 0 && R % K == 0, AIR_E_SHAPE);
    const int B = R / K;
    hipLaunchKernelGGL(iw_vimco_kernel, dim3(air_cdiv(B, 4)), dim3(256), 0, air_stream(stream), logw, K, B, bound, wnorm, signal, ess,
                       degenerate);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
