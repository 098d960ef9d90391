// Recovering objects a frame's parse missed from its neighbour frames, for gfx950 (include/air_hip.h states the rule):
//   air_temporal_pool: the candidate pool of C = T + P rows per frame: the T current rows followed by up to P rows of the frames
//                      f - 1 and f + 1 of the same sequence that no current object explains (float64 box IoU), ranked by score,
//                      greedily de-duplicated, optionally moved to the midpoint of the two sightings; the pool's presence chain, the
//                      provenance of every pool row, the count prior padded with zeros, and the state of every candidate.
// The search behind it is air_prune_score / air_prune_select unchanged, the provenance air_propose_source.
// Everything a float decides is float64 with contraction off; no atomics, no cross-workgroup traffic, one fixed order: the same bits
// run to run.
#include <math.h>
#include <limits.h>
#include "scene_device.h"

#define TEMPORAL_MAXT 6                  // PROPOSE_MAXT: air_prune_score is instantiated up to 6 rows
#define TEMPORAL_NONE 15u                // an empty 4-bit entry of the packed lists below (a candidate id is < 12)

enum { TEMPORAL_ABSENT = 0, TEMPORAL_TAKEN = 1, TEMPORAL_KNOWN = 2, TEMPORAL_DUPLICATE = 3, TEMPORAL_FULL = 4, TEMPORAL_NONFINITE = 5 };

struct TemporalPoolArgs {
    const float *what, *where, *glimpse, *score, *presence;       // the current rows [T, R, .] of ALL frames (Jacobi: only read)
    const int *n_in, *source_in;
    const double *prior;
    double iou_novel;
    float Hf, Wf;
    int round, T, P, F, R, A, G, both_sides, interpolate, what_vec, glimpse_vec;
    float *pool_what, *pool_where, *pool_glimpse, *pool_score, *pool_presence;
    int *pool_source;
    double *pool_prior;
    signed char *cand_state;
    int *taken, *partner;
};

// n of one row: the counts clipped to 0..T, else the leading ones of the presence chain (air_propose_pool's two forms); wave-uniform
__device__ __forceinline__ int temporal_count(const TemporalPoolArgs &a, int row, int lane) {
    if (a.n_in) {
        const int n = a.n_in[row];
        return n < 0 ? 0 : (n > a.T ? a.T : n);
    }
    const float z = lane < a.T ? a.presence[(size_t)lane * a.R + row] : 0.f;
    const unsigned long long present = __ballot(z > 0.5f);        // lanes >= T are clear: ~present is never 0
    return __ffsll((long long)~present) - 1;
}
// a where row of a buffer that is only known to be 4-byte aligned
__device__ __forceinline__ float4 temporal_where(const float *__restrict__ where, size_t k) {
    const float *p = where + 4 * k;
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ float4 temporal_shfl4(const float4 v, int src) {
    return make_float4(__shfl(v.x, src, 64), __shfl(v.y, src, 64), __shfl(v.z, src, 64), __shfl(v.w, src, 64));
}

// One wavefront per row r = s F + f.  Lane q < 2T owns candidate q (slot q of frame f - 1, slot q - T of frame f + 1): its box, its
// score, its state and its rank.  The walk in rank order is wave-uniform: the walked candidate's box and the taken ones' boxes travel
// by shuffle and every lane forms the same float64 IoU; the taken candidates and their partners are two packed lists of 4-bit ids in
// uniform registers (P <= 4).  Then the copies, all 64 lanes on the `what` and glimpse rows.
__global__ __launch_bounds__(256) void temporal_pool_kernel(TemporalPoolArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int T = a.T, P = a.P, F = a.F, R = a.R, A = a.A, G = a.G, C = T + P;
    if (r >= R) return;                                            // wave-uniform
    const int f = r % F;
    const bool has_prev = f > 0, has_next = f < F - 1 && a.both_sides != 0;      // never across a sequence boundary
    const int n = temporal_count(a, r, lane);
    const int n_prev = has_prev ? temporal_count(a, r - 1, lane) : 0;
    const int n_next = has_next ? temporal_count(a, r + 1, lane) : 0;
    // ---- the candidate of this lane ------------------------------------------------------------------------------------------
    const int side = lane >= T ? 1 : 0, slot = lane - side * T;
    const bool exists = lane < 2 * T && slot < (side ? n_next : n_prev);
    float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float sc = 0.f;
    if (exists) {
        const size_t ck = (size_t)slot * R + (side ? r + 1 : r - 1);
        w4 = temporal_where(a.where, ck);
        sc = a.score[ck];
    }
    const unsigned long long ex_mask = __ballot(exists);
    unsigned long long bad_mask = 0;                               // candidates with a non-finite `what` value
    for (int q = 0; q < 2 * T; ++q) {
        if (!((ex_mask >> q) & 1ull)) continue;                    // wave-uniform
        const int qs = q >= T ? 1 : 0;
        const float *row = a.what + ((size_t)(q - qs * T) * R + (qs ? r + 1 : r - 1)) * A;
        bool bad = false;
        for (int i = lane; i < A; i += 64) bad = bad || !isfinite(row[i]);
        if (__ballot(bad)) bad_mask |= 1ull << q;
    }
    const bool finite = isfinite(w4.x) && isfinite(w4.y) && isfinite(w4.z) && isfinite(w4.w) && isfinite(sc) &&
                        !((bad_mask >> lane) & 1ull);
    const float4 bq = attention_box4(w4, a.Wf, a.Hf);
    bool known = false;
    for (int j = 0; j < n; ++j) {                                  // the current objects' boxes: wave-uniform loads
        const float4 bj = attention_box4(temporal_where(a.where, (size_t)j * R + r), a.Wf, a.Hf);
        known = known || box_iou_f64(bq, bj) > a.iou_novel;   // a NaN comparison is false
    }
    int state = !exists ? TEMPORAL_ABSENT : (!finite ? TEMPORAL_NONFINITE : (known ? TEMPORAL_KNOWN : -1));
    const bool open = state < 0;
    // ---- rank: score descending, the lower q between equal scores (the open scores are finite) -----------------------------------
    int rank = 0;
    for (int p = 0; p < 2 * T; ++p) {
        const float sp = __shfl(sc, p, 64);
        const int op = __shfl((int)open, p, 64);
        if (op && (sp > sc || (sp == sc && p < lane))) ++rank;
    }
    const int n_open = __popcll(__ballot(open));
    // ---- the greedy walk (wave-uniform) --------------------------------------------------------------------------------------
    int n_taken = 0;
    unsigned taken_pack = 0u, partner_pack = 0xFFFFu;              // entry i: bits 4i .. 4i+3
    for (int k = 0; k < n_open; ++k) {
        const int c = __ffsll((long long)__ballot(open && rank == k)) - 1;       // exactly one lane has rank k
        const float4 bc = temporal_shfl4(bq, c);
        int dup = -1;
        for (int i = 0; i < n_taken; ++i) {
            const float4 bd = temporal_shfl4(bq, (int)((taken_pack >> (4 * i)) & 15u));
            if (dup < 0 && box_iou_f64(bc, bd) > a.iou_novel) dup = i;
        }
        int st;
        if (dup >= 0) {
            st = TEMPORAL_DUPLICATE;
            const int d = (int)((taken_pack >> (4 * dup)) & 15u);
            if ((c >= T) != (d >= T) && ((partner_pack >> (4 * dup)) & 15u) == TEMPORAL_NONE)      // the first one of the other side
                partner_pack = (partner_pack & ~(15u << (4 * dup))) | ((unsigned)c << (4 * dup));
        } else if (n_taken < P) {
            st = TEMPORAL_TAKEN;
            taken_pack |= (unsigned)c << (4 * n_taken);
            ++n_taken;
        } else {
            st = TEMPORAL_FULL;
        }
        if (lane == c) state = st;
    }
    // ---- diagnostics, presence, provenance, prior ------------------------------------------------------------------------------
    if (lane < 2 * T) a.cand_state[(size_t)r * (2 * T) + lane] = (signed char)state;
    if (lane == 0) a.taken[r] = n_taken;
    if (lane < P) {
        const unsigned pp = (partner_pack >> (4 * lane)) & 15u;
        a.partner[(size_t)lane * R + r] = (lane < n_taken && pp != TEMPORAL_NONE) ? (int)pp : -1;
    }
    if (lane < C) {
        const size_t k = (size_t)lane * R + r;
        a.pool_presence[k] = lane < n ? 1.f : 0.f;
        int src;
        if (lane < T) src = a.source_in ? a.source_in[k] : lane;
        else src = lane - T < n_taken ? T + a.round * 2 * T + (int)((taken_pack >> (4 * (lane - T))) & 15u) : -1;
        a.pool_source[k] = src;
    }
    if (r == 0 && lane <= C) a.pool_prior[lane] = lane <= T ? a.prior[lane] : 0.0;
    // ---- the C pool rows of this frame ---------------------------------------------------------------------------------------------
    const unsigned *where_u = reinterpret_cast<const unsigned *>(a.where), *score_u = reinterpret_cast<const unsigned *>(a.score);
    unsigned *pwhere_u = reinterpret_cast<unsigned *>(a.pool_where), *pscore_u = reinterpret_cast<unsigned *>(a.pool_score);
    for (int j = 0; j < C; ++j) {
        const size_t to = (size_t)j * R + r;
        if (j >= T + n_taken) {                                    // an unused proposal row: a NaN joint in every subset that has it
            if (lane < 4) pwhere_u[to * 4 + lane] = __float_as_uint((lane & 1) ? 0.f : 1.f);
            if (lane == 4) pscore_u[to] = 0u;
            fill_row_bits(a.pool_what + to * A, A, a.what_vec != 0, lane, 0x7fc00000u);
            fill_row_bits(a.pool_glimpse + to * G, G, a.glimpse_vec != 0, lane, 0u);
            continue;
        }
        size_t from = to, mate = 0;
        bool mid = false;
        if (j >= T) {
            const int d = (int)((taken_pack >> (4 * (j - T))) & 15u), ds = d >= T ? 1 : 0;
            from = (size_t)(d - ds * T) * R + (ds ? r + 1 : r - 1);
            const unsigned pp = (partner_pack >> (4 * (j - T))) & 15u;
            if (a.interpolate != 0 && pp != TEMPORAL_NONE) {       // the partner is of the other side
                mid = true;
                mate = (size_t)((int)pp - (1 - ds) * T) * R + (ds ? r - 1 : r + 1);
            }
        }
        if (lane < 4) {
            unsigned bits = where_u[from * 4 + lane];
            if (mid) {
                const double wd = (double)__uint_as_float(bits), wc = (double)a.where[mate * 4 + lane];
                bits = __float_as_uint((float)(0.5 * (wd + wc)));
            }
            pwhere_u[to * 4 + lane] = bits;
        }
        if (lane == 4) pscore_u[to] = score_u[from];
        copy_row_bits(a.what + from * A, a.pool_what + to * A, A, a.what_vec != 0, lane);
        copy_row_bits(a.glimpse + from * G, a.pool_glimpse + to * G, G, a.glimpse_vec != 0, lane);
    }
}

extern "C" int air_temporal_pool(const float *what, const float *where, const float *glimpse, const float *score, const float *presence,
                                 const int *num_objects_in, const int *source_in, const double *prior_f64, int round, int T, int P,
                                 int S, int F, int A, int G, int H, int W, double iou_novel, int both_sides, int interpolate,
                                 float *pool_what, float *pool_where, float *pool_glimpse, float *pool_score, float *pool_presence,
                                 int *pool_source, double *pool_prior, signed char *cand_state, int *taken, int *partner,
                                 void *stream) {
    AIR_REQUIRE(what && where && glimpse && score && (presence || num_objects_in) && prior_f64 && pool_what && pool_where &&
                pool_glimpse && pool_score && pool_presence && pool_source && pool_prior && cand_state && taken && partner, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= TEMPORAL_MAXT && P > 0 && P <= 2 * T && P <= TEMPORAL_MAXT - T, AIR_E_SHAPE);
    AIR_REQUIRE(S > 0 && F > 0 && A > 0 && G > 0 && H > 0 && W > 0 && round >= 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)S * F <= (long)INT_MAX && (long)T + ((long)round + 1) * 2 * T <= (long)INT_MAX, AIR_E_SHAPE);
    const uintptr_t all = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(where) | reinterpret_cast<uintptr_t>(glimpse) |
                          reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(presence) |
                          reinterpret_cast<uintptr_t>(num_objects_in) | reinterpret_cast<uintptr_t>(source_in) |
                          reinterpret_cast<uintptr_t>(pool_what) | reinterpret_cast<uintptr_t>(pool_where) |
                          reinterpret_cast<uintptr_t>(pool_glimpse) | reinterpret_cast<uintptr_t>(pool_score) |
                          reinterpret_cast<uintptr_t>(pool_presence) | reinterpret_cast<uintptr_t>(pool_source) |
                          reinterpret_cast<uintptr_t>(taken) | reinterpret_cast<uintptr_t>(partner);
    const uintptr_t dbl = reinterpret_cast<uintptr_t>(prior_f64) | reinterpret_cast<uintptr_t>(pool_prior);
    AIR_REQUIRE((all & 3u) == 0 && (dbl & 7u) == 0, AIR_E_ALIGN);
    const int R = S * F;
    const TemporalPoolArgs a = {what, where, glimpse, score, presence, num_objects_in, source_in, prior_f64, iou_novel, (float)H, (float)W,
                                round, T, P, F, R, A, G, both_sides, interpolate,
                                A % 4 == 0 && air_aligned16(what) && air_aligned16(pool_what),
                                G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(pool_glimpse),
                                pool_what, pool_where, pool_glimpse, pool_score, pool_presence, pool_source, pool_prior, cand_state,
                                taken, partner};
    hipLaunchKernelGGL(temporal_pool_kernel, dim3(air_cdiv(R, 4)), dim3(256), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
