// The generative half of AIR for gfx950: scenes drawn from p(n) p(what) p(where) p(x | z) (model.py:92-97,126-216, cell.py:158-165).
//   air_prior_latents: the ancestral draw of the latents of R scenes from caller-supplied noise -- the object count by inversion of
//                      a float64 count table, the monotone chain of presences it implies, what / where from their Gaussian priors;
//   air_observe:       the observation model x ~ N(mult * canvas, std) at dataset scale: the pixel noise is drawn in registers
//                      (Philox4x32-10, the numbers air_rng_fill would write), no noise buffer exists.
// Decoder and canvas in between are the entries the train step uses (air_linear_fwd / air_gemm_bf16, air_canvas_unroll_fwd).
#include <math.h>
#include "scene_device.h"
#include "engine_device.h"
#include "prologue_device.h"

#define GEN_MAXT 32

struct GenPriors {
    float what_loc, what_scale, scale_loc, scale_scale, shift_loc, shift_scale;
};

// One wavefront per scene (row r).  Every lane forms the same count n (T + 1 float64 adds in index order: the table is tiny
// and wave-uniform), lane t < T then writes presence[t, r] and the four `where` components of step t, and the T A-wide
// `what` rows are spread over the lanes as T * A / V vectors of V floats (V = 4 / 2 / 1: what the row starts allow).
// Latents of absent steps are written like the others: inference draws them too, the presence masks them.
template <int V>
__global__ __launch_bounds__(256) void prior_latents_kernel(
    const double *__restrict__ table, const float *__restrict__ u_n, const int *__restrict__ n_in,
    const float *__restrict__ eps_what, const float *__restrict__ eps_where, GenPriors pr, float guard, int T, int R, int A,
    float *__restrict__ what, float *__restrict__ where, float *__restrict__ presence, int *__restrict__ n_out) {
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform

    int n;
    if (n_in) {
        n = n_in[r];
        n = n < 0 ? 0 : (n > T ? T : n);
    } else {
        // inversion of the (unnormalised) table: n = #{c < T : cum_c <= u * total}.  cum is non-decreasing, so the c that
        // count are a prefix; a weight of exactly zero adds nothing to cum and is stepped over, also at u = 0
        double total = 0.0;
        for (int c = 0; c <= T; ++c) total += table[c];
        const double thresh = (double)u_n[r] * total;
        double cum = 0.0;
        n = 0;
        for (int c = 0; c < T; ++c) {
            cum += table[c];
            n += cum <= thresh ? 1 : 0;
        }
    }
    if (lane == 0) n_out[r] = n;
    if (lane < T) {
        presence[(size_t)lane * R + r] = lane < n ? 1.f : 0.f;
        const size_t off = ((size_t)lane * R + r) * 4;
        const float4 e = *reinterpret_cast<const float4 *>(eps_where + off);
        float4 w;                                                  // [sx, tx, sy, ty]: scale prior on 0, 2, shift prior on 1, 3
        w.x = guard_where(pr.scale_loc + pr.scale_scale * e.x, 0, 1, guard);
        w.y = pr.shift_loc + pr.shift_scale * e.y;
        w.z = guard_where(pr.scale_loc + pr.scale_scale * e.z, 2, 1, guard);
        w.w = pr.shift_loc + pr.shift_scale * e.w;
        *reinterpret_cast<float4 *>(where + off) = w;
    }
    const int AV = A / V, items = T * AV;
    for (int j = lane; j < items; j += 64) {
        const int t = j / AV, i = j - t * AV;
        const size_t off = ((size_t)t * R + r) * A + (size_t)i * V;
        const vec_t e = *reinterpret_cast<const vec_t *>(eps_what + off);
        vec_t x;
        const float *ef = reinterpret_cast<const float *>(&e);
        float *xf = reinterpret_cast<float *>(&x);
#pragma unroll
        for (int v = 0; v < V; ++v) xf[v] = pr.what_loc + pr.what_scale * ef[v];
        *reinterpret_cast<vec_t *>(what + off) = x;
    }
}

// ---- observation model -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gen_clamp(float v, float lo, float hi) {
    if (lo == lo) v = fmaxf(v, lo);                                // a NaN bound: no clamp on that side
    if (hi == hi) v = fminf(v, hi);
    return v;
}

typedef float gen_f4 __attribute__((ext_vector_type(4)));

// One thread per quad of four adjacent pixels = one Philox call = the quad air_rng_fill's thread q writes (same counter, stream
// id 0, same Box-Muller pairing: prologue_device.h).  VEC: every pointer is 16-byte aligned, complete quads move as one 16-byte
// load and one (non-temporal: nothing on the chip reads a dataset-sized output back) 16-byte store per output; the last,
// incomplete quad and unaligned buffers take the scalar form.  NOISE = false (std == 0): no draw, obs = mean bit for bit.
template <bool VEC, bool NOISE>
__global__ __launch_bounds__(PW_THREADS) void observe_kernel(const float *__restrict__ canvas, float mult, float std,
                                                             const uint64_t *__restrict__ state, uint64_t counter_base,
                                                             float lo, float hi, float *__restrict__ mean_out,
                                                             float *__restrict__ obs_out, size_t n) {
    const size_t nq = (n + 3) / 4;
    uint64_t seed = 0, base = 0;
    if (NOISE) {
        seed = state[0];
        base = state[1] + counter_base;
    }
    for (size_t q = (size_t)blockIdx.x * PW_THREADS + threadIdx.x; q < nq; q += (size_t)gridDim.x * PW_THREADS) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISE) {
            uint32_t rr[4];
            philox4x32(base + q, 0, seed, rr);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float rad = sqrtf(-2.0f * logf(u01_open(rr[2 * k])));
                float sn, cs;
                sincosf(6.283185307179586f * u01(rr[2 * k + 1]), &sn, &cs);
                z[2 * k] = rad * cs; z[2 * k + 1] = rad * sn;
            }
        }
        if (VEC && 4 * q + 3 < n) {
            const gen_f4 c = __builtin_nontemporal_load(reinterpret_cast<const gen_f4 *>(canvas) + q);
            const gen_f4 m = {mult * c.x, mult * c.y, mult * c.z, mult * c.w};
            if (mean_out) __builtin_nontemporal_store(m, reinterpret_cast<gen_f4 *>(mean_out) + q);
            if (obs_out) {
                gen_f4 o = m;
                if (NOISE) {
                    o.x = m.x + std * z[0]; o.y = m.y + std * z[1]; o.z = m.z + std * z[2]; o.w = m.w + std * z[3];
                }
                o.x = gen_clamp(o.x, lo, hi); o.y = gen_clamp(o.y, lo, hi); o.z = gen_clamp(o.z, lo, hi); o.w = gen_clamp(o.w, lo, hi);
                __builtin_nontemporal_store(o, reinterpret_cast<gen_f4 *>(obs_out) + q);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t i = 4 * q + k;
                if (i < n) {
                    const float m = mult * canvas[i];
                    if (mean_out) mean_out[i] = m;
                    if (obs_out) obs_out[i] = gen_clamp(NOISE ? m + std * z[k] : m, lo, hi);
                }
            }
        }
    }
}

extern "C" int air_prior_latents(const double *count_table_f64, const float *u_n, const int *num_objects_in, const float *eps_what,
                                 const float *eps_where, float what_p_loc, float what_p_scale, float scale_p_loc,
                                 float scale_p_scale, float shift_p_loc, float shift_p_scale, float guard_eps, int T, int R, int A,
                                 float *what, float *where, float *presence, int *num_objects, void *stream) {
    AIR_REQUIRE(eps_what && eps_where && what && where && presence && num_objects, AIR_E_NULL);
    AIR_REQUIRE(num_objects_in || (count_table_f64 && u_n), AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= GEN_MAXT && R > 0 && A > 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(eps_where) && air_aligned16(where), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(eps_what) | reinterpret_cast<uintptr_t>(what);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const GenPriors pr = {what_p_loc, what_p_scale, scale_p_loc, scale_p_scale, shift_p_loc, shift_p_scale};
    const dim3 grid(air_cdiv(R, 4)), block(256);
#define GEN_LAUNCH(V)                                                                                                              \
    hipLaunchKernelGGL(prior_latents_kernel<V>, grid, block, 0, air_stream(stream), count_table_f64, u_n, num_objects_in, eps_what, \
                       eps_where, pr, guard_eps, T, R, A, what, where, presence, num_objects)
    if (A % 4 == 0 && (bits & 15u) == 0) GEN_LAUNCH(4);
    else if (A % 2 == 0 && (bits & 7u) == 0) GEN_LAUNCH(2);
    else GEN_LAUNCH(1);
#undef GEN_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_observe(const float *canvas, float mult, float std, const uint64_t *state_dev, uint64_t counter_base,
                           float clamp_lo, float clamp_hi, float *mean_out, float *obs_out, size_t n, void *stream) {
    AIR_REQUIRE(canvas && (mean_out || obs_out), AIR_E_NULL);
    const bool noise = std != 0.f && obs_out;
    AIR_REQUIRE(!noise || state_dev, AIR_E_NULL);
    AIR_REQUIRE(n > 0, AIR_E_SHAPE);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(canvas) | reinterpret_cast<uintptr_t>(mean_out) |
                           reinterpret_cast<uintptr_t>(obs_out);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const bool vec = (bits & 15u) == 0;
    const size_t nq = (n + 3) / 4;
    const dim3 grid(prologue_pw_blocks(nq)), block(PW_THREADS);
#define GEN_LAUNCH(VEC, NOISE)                                                                                                   \
    hipLaunchKernelGGL((observe_kernel<VEC, NOISE>), grid, block, 0, air_stream(stream), canvas, mult, std, state_dev, counter_base, \
                       clamp_lo, clamp_hi, mean_out, obs_out, n)
    if (vec && noise) GEN_LAUNCH(true, true);
    else if (vec) GEN_LAUNCH(true, false);
    else if (noise) GEN_LAUNCH(false, true);
    else GEN_LAUNCH(false, false);
#undef GEN_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
