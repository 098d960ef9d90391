// Parsing scenes larger than the model's canvas for gfx950: overlapping windows in, one merged object list per scene out.
//   air_tile_gather:  scenes[S,Hs,Ws] -> windows[S*Nw, H*W], window (i, j) of a scene at origin (min(i*sy, Hs-H), min(j*sx, Ws-W)):
//                     a pure copy, one workgroup per (window, row band), 16-byte moves where the window's rows allow them;
//   air_tile_merge:   per scene the Nw*T per-window objects lifted into the scene frame (float64), ownership by box centre,
//                     greedy suppression of what two windows both saw (by score, float64 box IoU), the survivors compacted into
//                     leading rows that air_parse_objects / air_parse_render take with T := C, R := S;
//   air_tile_relabel: air_prune_relabel's rule for up to 32 rows (that entry stops at the 6 steps subset pruning enumerates).
// No atomics, no cross-workgroup traffic, one fixed order: the same bits run to run.
#include <math.h>
#include <limits.h>
#include "scene_device.h"

#define TILE_THREADS 256
#define TILE_MAXC 32                     // PARSE_MAXT / SCORE_MAXT: the slots of a merged scene
#define TILE_MAXCAND 256                 // candidates per scene: one thread each
#define TILE_BAND_FLOATS 2048            // a gather workgroup moves about this many floats

enum { TILE_ABSENT = 0, TILE_KEPT = 1, TILE_NOT_OWNED = 2, TILE_DUPLICATE = 3, TILE_OVERFLOW = 4, TILE_NONFINITE = 5 };

static inline int tile_count(int scene, int window, int stride) { return 1 + (scene - window + stride - 1) / stride; }
__host__ __device__ __forceinline__ int tile_origin(int i, int stride, int last) { return i * stride < last ? i * stride : last; }

// ============================================================================================================
// gather
// ============================================================================================================
struct TileGatherArgs {
    const float *scenes;
    float *windows;
    int Hs, Ws, H, W, sy, sx, ny, nx, NB, RB, aligned;
};

// One workgroup per (window row r = s * Nw + i * nx + j, band of RB window rows).  Whether the 16-byte path can be taken is decided
// per window (ox decides it, with Ws, W and the two bases): uniform over the workgroup.
__global__ __launch_bounds__(TILE_THREADS) void tile_gather_kernel(TileGatherArgs a) {
    const int H = a.H, W = a.W, Ws = a.Ws, Nw = a.ny * a.nx;
    const int unit = blockIdx.x;                                   // < S * Nw * NB: the grid is exactly the units
    const int r = unit / a.NB, band = unit - r * a.NB;
    const int s = r / Nw, v = r - s * Nw, i = v / a.nx, j = v - i * a.nx;
    const int oy = tile_origin(i, a.sy, a.Hs - H), ox = tile_origin(j, a.sx, Ws - W);
    const int r0 = band * a.RB, r1 = r0 + a.RB < H ? r0 + a.RB : H;
    const float *__restrict__ src = a.scenes + ((size_t)s * a.Hs + (size_t)(oy + r0)) * Ws + ox;
    float *__restrict__ dst = a.windows + ((size_t)r * H + r0) * W;
    const int tid = threadIdx.x;
    if (a.aligned && (ox & 3) == 0) {                              // every row starts on 16 bytes in the scene and in the window
        const int W4 = W >> 2, n4 = (r1 - r0) * W4;
        for (int e = tid; e < n4; e += TILE_THREADS) {
            const int row = e / W4, q = e - row * W4;
            reinterpret_cast<uint4 *>(dst + (size_t)row * W)[q] = reinterpret_cast<const uint4 *>(src + (size_t)row * Ws)[q];
        }
    } else {
        const int n = (r1 - r0) * W;
        for (int e = tid; e < n; e += TILE_THREADS) {
            const int row = e / W, q = e - row * W;
            reinterpret_cast<unsigned *>(dst)[e] = reinterpret_cast<const unsigned *>(src + (size_t)row * Ws)[q];
        }
    }
}

static inline int tile_check_geometry(int S, int Hs, int Ws, int H, int W, int sy, int sx, int *ny, int *nx) {
    AIR_REQUIRE(S > 0 && H > 1 && W > 1 && Hs >= H && Ws >= W, AIR_E_SHAPE);
    AIR_REQUIRE(sy >= 1 && sy <= H && sx >= 1 && sx <= W, AIR_E_SHAPE);
    AIR_REQUIRE((long)Hs * Ws <= (long)INT_MAX / 2, AIR_E_SHAPE);
    *ny = tile_count(Hs, H, sy);
    *nx = tile_count(Ws, W, sx);
    AIR_REQUIRE((long)*ny * *nx <= (long)INT_MAX && (long)S * *ny * *nx <= (long)INT_MAX, AIR_E_SHAPE);
    return AIR_OK;
}

extern "C" int air_tile_gather(const float *scenes, int S, int Hs, int Ws, int H, int W, int sy, int sx, float *windows,
                               void *stream) {
    AIR_REQUIRE(scenes && windows, AIR_E_NULL);
    int ny, nx;
    const int st = tile_check_geometry(S, Hs, Ws, H, W, sy, sx, &ny, &nx);
    if (st) return st;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(scenes) | reinterpret_cast<uintptr_t>(windows);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    int RB = air_cdiv(TILE_BAND_FLOATS, W);
    RB = RB < 1 ? 1 : (RB > H ? H : RB);
    const int NB = air_cdiv(H, RB);
    AIR_REQUIRE((long)S * ny * nx * NB <= (long)INT_MAX, AIR_E_SHAPE);
    const TileGatherArgs a = {scenes, windows, Hs, Ws, H, W, sy, sx, ny, nx, NB, RB,
                              ((bits & 15u) == 0 && W % 4 == 0 && Ws % 4 == 0 && ((long)Hs * Ws) % 4 == 0) ? 1 : 0};
    hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)((long)S * ny * nx * NB)), dim3(TILE_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// merge
// ============================================================================================================
struct TileMergeArgs {
    const float *what, *where, *glimpse, *score;
    const int *num_objects;
    float *what_out, *where_out, *glimpse_out, *score_out;
    int *kept_cand, *num_objects_out, *dup_of, *merge_counts;
    signed char *cand_state;
    double iou_merge;
    int T, S, A, G, Hs, Ws, H, W, sy, sx, ny, nx, C, what_vec, glimpse_vec;
};

// one axis of the lift: (scale, shift) of a window at origin o -> the scene frame, float64, rounded once by the caller
__device__ __forceinline__ void tile_lift_axis(float sc, float sh, int scene, int window, int o, double *sc_out, double *sh_out) {
#pragma clang fp contract(off)
    const double a = (double)(scene - 1) / (double)(window - 1);
    const double b = (a - 1.0) - (2.0 * (double)o) / (double)(window - 1);
    *sc_out = (double)sc / a;
    *sh_out = ((double)sh - b) / a;
}

// is the centre c inside the cell of window i (of n, origins by tile_origin)?  Cells are half open: [beta_{i-1}, beta_i)
__device__ __forceinline__ bool tile_owns(double c, int i, int n, int stride, int last, int window) {
#pragma clang fp contract(off)
    bool in = true;
    if (i > 0) in = in && c >= (double)(tile_origin(i, stride, last) + tile_origin(i - 1, stride, last) + window) / 2.0;
    if (i < n - 1) in = in && c < (double)(tile_origin(i + 1, stride, last) + tile_origin(i, stride, last) + window) / 2.0;
    return in;
}

// the kept rows of one table, copied by the whole workgroup: slot-major items of V words
template <int V>
__device__ __forceinline__ void tile_copy_rows(const float *__restrict__ src, float *__restrict__ dst, int n, int len, int R, int S,
                                               int s, int Nw, int T, const int *slot_cand, int tid) {
    typedef typename VecOf<V>::type vec_t;
    const int LV = len / V, items = n * LV;
    for (int e = tid; e < items; e += TILE_THREADS) {
        const int slot = e / LV, q = e - slot * LV, c = slot_cand[slot], v = c / T, t = c - v * T;
        const size_t from = ((size_t)t * R + (size_t)s * Nw + v) * len, to = ((size_t)slot * S + s) * len;
        reinterpret_cast<vec_t *>(dst + to)[q] = reinterpret_cast<const vec_t *>(src + from)[q];
    }
}

// One 256-thread workgroup per scene, thread c = candidate c = v * T + t (window v, step t).
__global__ __launch_bounds__(TILE_THREADS) void tile_merge_kernel(TileMergeArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 box_s[TILE_MAXCAND];
    __shared__ float score_s[TILE_MAXCAND];
    __shared__ int order_s[TILE_MAXCAND];                          // walk position -> candidate
    __shared__ int sup_s[TILE_MAXCAND];                            // suppressor of a candidate, -1 = none
    __shared__ unsigned char owned_s[TILE_MAXCAND], kept_s[TILE_MAXCAND];
    __shared__ int wave_s[TILE_THREADS / 64][8];                   // per wave: the six state counts, owned, kept
    __shared__ int slot_cand_s[TILE_MAXC];
    const int T = a.T, S = a.S, Nw = a.ny * a.nx, Nc = Nw * T, R = S * Nw, C = a.C;
    const int s = blockIdx.x, c = threadIdx.x, lane = c & 63, wid = c >> 6;
    const bool live = c < Nc;
    const int v = live ? c / T : 0, t = live ? c - v * T : 0, wi = v / a.nx, wj = v - wi * a.nx;
    const int r = s * Nw + v;
    const int oy = tile_origin(wi, a.sy, a.Hs - a.H), ox = tile_origin(wj, a.sx, a.Ws - a.W);

    // ---- lift, finiteness, ownership ---------------------------------------------------------------------------------------
    int state = TILE_ABSENT;
    float4 lifted = make_float4(0.f, 0.f, 0.f, 0.f), box = make_float4(0.f, 0.f, 0.f, 0.f);
    float sc = 0.f;
    if (live && t < a.num_objects[r]) {
        const size_t k = (size_t)t * R + r;
        const float4 w4 = *reinterpret_cast<const float4 *>(a.where + 4 * k);    // [sx, tx, sy, ty]
        sc = a.score[k];
        double lsx, ltx, lsy, lty;
        tile_lift_axis(w4.x, w4.y, a.Ws, a.W, ox, &lsx, &ltx);
        tile_lift_axis(w4.z, w4.w, a.Hs, a.H, oy, &lsy, &lty);
        lifted = make_float4((float)lsx, (float)ltx, (float)lsy, (float)lty);
        const float Wf = (float)a.Ws, Hf = (float)a.Hs;            // evaluation.attention_box as air_parse_objects forms it
        box.x = Wf * ((1.f - lifted.x) + lifted.y) * 0.5f;
        box.y = Hf * ((1.f - lifted.z) + lifted.w) * 0.5f;
        box.z = Wf * lifted.x;
        box.w = Hf * lifted.z;
        const bool finite = isfinite(lifted.x) && isfinite(lifted.y) && isfinite(lifted.z) && isfinite(lifted.w) && isfinite(sc);
        if (!finite) {
            state = TILE_NONFINITE;
        } else {
            const double cx = ((double)a.Ws * (1.0 + (double)lifted.y)) / 2.0, cy = ((double)a.Hs * (1.0 + (double)lifted.w)) / 2.0;
            const bool mine = tile_owns(cx, wj, a.nx, a.sx, a.Ws - a.W, a.W) && tile_owns(cy, wi, a.ny, a.sy, a.Hs - a.H, a.H);
            state = mine ? TILE_KEPT : TILE_NOT_OWNED;             // (owned: settled by the walk below)
        }
    }
    const bool owned = state == TILE_KEPT;
    box_s[c] = box;
    score_s[c] = sc;
    owned_s[c] = owned ? 1 : 0;
    kept_s[c] = 0;
    sup_s[c] = -1;
    {
        const int n_owned_wave = __popcll(__ballot(owned));
        if (lane == 0) wave_s[wid][6] = n_owned_wave;
    }
    __syncthreads();
    int n_owned = 0;
#pragma unroll
    for (int k = 0; k < TILE_THREADS / 64; ++k) n_owned += wave_s[k][6];

    // ---- the walk order: score descending, the lower candidate first between equal scores ------------------------------------
    if (owned) {
        int rank = 0;
        for (int o = 0; o < Nc; ++o) {
            const float so = score_s[o];
            rank += (owned_s[o] && (so > sc || (so == sc && o < c))) ? 1 : 0;
        }
        order_s[rank] = c;
    }
    __syncthreads();

    // ---- the greedy walk: a candidate nobody suppressed is kept and suppresses, at once, what it overlaps in other windows --------
    int n_kept = 0;
    for (int k = 0; k < n_owned && n_kept < C; ++k) {
        const int ck = order_s[k];                                 // workgroup-uniform, as is the test below
        if (sup_s[ck] >= 0) continue;
        if (c == ck) kept_s[c] = 1;
        ++n_kept;
        if (owned && c != ck && ck / T != v && sup_s[c] < 0 && !kept_s[c] && box_iou_f64(box_s[ck], box) > a.iou_merge) sup_s[c] = ck;
        __syncthreads();
    }
    __syncthreads();
    if (owned) state = sup_s[c] >= 0 ? TILE_DUPLICATE : (kept_s[c] ? TILE_KEPT : TILE_OVERFLOW);
    const bool kept = state == TILE_KEPT;

    // ---- counts and slots: a prefix count over candidate ids -----------------------------------------------------------------
    const unsigned long long kept_mask = __ballot(kept);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int n = __popcll(__ballot(live && state == q));
        if (lane == 0) wave_s[wid][q] = n;
    }
    if (lane == 0) wave_s[wid][7] = __popcll(kept_mask);
    __syncthreads();
    int slot = __popcll(kept_mask & ((1ull << lane) - 1ull));
    for (int k = 0; k < wid; ++k) slot += wave_s[k][7];
    if (kept) slot_cand_s[slot] = c;
    if (live) {
        a.cand_state[(size_t)s * Nc + c] = (signed char)state;
        a.dup_of[(size_t)s * Nc + c] = state == TILE_DUPLICATE ? sup_s[c] : -1;
    }
    if (c < 6) {
        int n = 0;
#pragma unroll
        for (int k = 0; k < TILE_THREADS / 64; ++k) n += wave_s[k][c];
        a.merge_counts[(size_t)s * 6 + c] = n;
    }
    if (c == 0) a.num_objects_out[s] = n_kept;
    if (c >= n_kept && c < C) a.kept_cand[(size_t)c * S + s] = -1;
    if (kept) {
        const size_t to = (size_t)slot * S + s;
        *reinterpret_cast<float4 *>(a.where_out + 4 * to) = lifted;
        reinterpret_cast<unsigned *>(a.score_out)[to] = __float_as_uint(sc);
        a.kept_cand[to] = c;
    }
    __syncthreads();

    // ---- bit copies of the kept what / glimpse rows ------------------------------------------------------------------------------
    if (a.what_vec) tile_copy_rows<4>(a.what, a.what_out, n_kept, a.A, R, S, s, Nw, T, slot_cand_s, c);
    else tile_copy_rows<1>(a.what, a.what_out, n_kept, a.A, R, S, s, Nw, T, slot_cand_s, c);
    if (a.glimpse_vec) tile_copy_rows<4>(a.glimpse, a.glimpse_out, n_kept, a.G, R, S, s, Nw, T, slot_cand_s, c);
    else tile_copy_rows<1>(a.glimpse, a.glimpse_out, n_kept, a.G, R, S, s, Nw, T, slot_cand_s, c);
}

extern "C" int air_tile_merge(const float *what, const float *where, const float *glimpse, const float *score, const int *num_objects,
                              int T, int S, int A, int G, int Hs, int Ws, int H, int W, int sy, int sx, double iou_merge,
                              float *what_out, float *where_out, float *glimpse_out, float *score_out, int *kept_cand,
                              int *num_objects_out, signed char *cand_state, int *dup_of, int *merge_counts, void *stream) {
    AIR_REQUIRE(what && where && glimpse && score && num_objects && what_out && where_out && glimpse_out && score_out && kept_cand &&
                num_objects_out && cand_state && dup_of && merge_counts, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= TILE_MAXC && A > 0 && G > 0, AIR_E_SHAPE);
    int ny, nx;
    const int st = tile_check_geometry(S, Hs, Ws, H, W, sy, sx, &ny, &nx);
    if (st) return st;
    AIR_REQUIRE((long)ny * nx * T <= TILE_MAXCAND, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(where_out), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(score) |
                           reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(what_out) |
                           reinterpret_cast<uintptr_t>(glimpse_out) | reinterpret_cast<uintptr_t>(score_out) |
                           reinterpret_cast<uintptr_t>(kept_cand) | reinterpret_cast<uintptr_t>(num_objects_out) |
                           reinterpret_cast<uintptr_t>(dup_of) | reinterpret_cast<uintptr_t>(merge_counts);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const int Nc = ny * nx * T;
    const TileMergeArgs a = {what, where, glimpse, score, num_objects, what_out, where_out, glimpse_out, score_out, kept_cand,
                             num_objects_out, dup_of, merge_counts, cand_state, iou_merge, T, S, A, G, Hs, Ws, H, W, sy, sx, ny, nx,
                             Nc < TILE_MAXC ? Nc : TILE_MAXC,
                             (A % 4 == 0 && air_aligned16(what) && air_aligned16(what_out)) ? 1 : 0,
                             (G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(glimpse_out)) ? 1 : 0};
    hipLaunchKernelGGL(tile_merge_kernel, dim3((unsigned)S), dim3(TILE_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// relabel
// ============================================================================================================
// The kernel is parse_relabel_kernel (parse_kernels.hip); this entry takes up to the 32 slots of a merged scene.
extern "C" int air_tile_relabel(const float *score_src, const int *kept_cand, const int *num_objects, const int *offsets, int C,
                                int S, float *score, float *obj_score, int *obj_step, void *stream) {
    AIR_REQUIRE(score_src && kept_cand && num_objects && offsets && score && obj_score && obj_step, AIR_E_NULL);
    AIR_REQUIRE(C > 0 && C <= TILE_MAXC && S > 0, AIR_E_SHAPE);
    const uintptr_t all = reinterpret_cast<uintptr_t>(score_src) | reinterpret_cast<uintptr_t>(kept_cand) |
                          reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(offsets) |
                          reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(obj_score) | reinterpret_cast<uintptr_t>(obj_step);
    AIR_REQUIRE((all & 3u) == 0, AIR_E_ALIGN);
    return parse_relabel_launch(score_src, kept_cand, num_objects, offsets, C, S, score, obj_score, obj_step, stream);
}
