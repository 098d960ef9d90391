// Device and host helpers shared by the scene read-outs behind a forward pass (parse, particle, refine, prune, propose, tile, track,
// temporal, trajectory, score; iw and gen take the vector type and the butterflies).  These are contracts between kernels: a stage
// that promises "air_score_match's box IoU" or "air_parse_render's bits" keeps the promise by calling the function the other stage
// calls -- one IoU, one row copy, one band staging, one relabel (parse_kernels.hip).  Every function whose bits matter carries its own
// `#pragma clang fp contract(off)`, so it keeps them when it is inlined into a translation unit that contracts.
#pragma once
#include "st_device.h"

// V floats as one load / store: what a row's length and start allow
template <int V> struct VecOf;
template <> struct VecOf<4> { typedef float4 type; };
template <> struct VecOf<2> { typedef float2 type; };
template <> struct VecOf<1> { typedef float type; };

#define HALF_LOG_2PI 0.91893853320467274178f
// log N(x | loc, scale), log_scale = logf(scale).  No clamps: a zero scale gives the +-inf / NaN of the plain formula.
__device__ __forceinline__ float log_normal(float x, float loc, float scale, float log_scale) {
    const float z = (x - loc) / scale;
    return -0.5f * (z * z) - log_scale - HALF_LOG_2PI;
}

// air_score_match's float64 box IoU of two (left, top, width, height) boxes
__device__ __forceinline__ double box_iou_f64(const float4 a, const float4 b) {
#pragma clang fp contract(off)
    const double al = (double)a.x, at = (double)a.y, ar = (double)a.x + (double)a.z, ab = (double)a.y + (double)a.w;
    const double bl = (double)b.x, bt = (double)b.y, br = (double)b.x + (double)b.z, bb = (double)b.y + (double)b.w;
    const double ax0 = fmin(al, ar), ax1 = fmax(al, ar), ay0 = fmin(at, ab), ay1 = fmax(at, ab);
    const double bx0 = fmin(bl, br), bx1 = fmax(bl, br), by0 = fmin(bt, bb), by1 = fmax(bt, bb);
    // a NaN coordinate must score 0: fmin / fmax drop a NaN operand, so it is tested for on its own
    const bool nan = (a.x != a.x) || (a.y != a.y) || (a.z != a.z) || (a.w != a.w) || (b.x != b.x) || (b.y != b.y) ||
                     (b.z != b.z) || (b.w != b.w);
    const double iw = fmax(0.0, fmin(ax1, bx1) - fmax(ax0, bx0)), ih = fmax(0.0, fmin(ay1, by1) - fmax(ay0, by0));
    const double inter = iw * ih;
    const double uni = ((ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0)) - inter;
    const double q = inter / uni;
    return (!nan && inter > 0.0 && uni > 0.0 && isfinite(q)) ? q : 0.0;
}

// ---- one row of n floats moved as bits by the 64 lanes of a wave; vec: 16-byte vectors (n % 4 == 0 and the buffers start aligned) ----
__device__ __forceinline__ void copy_row_bits(const float *__restrict__ src, float *__restrict__ dst, int n, bool vec, int lane) {
    if (vec) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int i = lane; i < n / 4; i += 64) d4[i] = s4[i];
    } else {
        const unsigned *s1 = reinterpret_cast<const unsigned *>(src);
        unsigned *d1 = reinterpret_cast<unsigned *>(dst);
        for (int i = lane; i < n; i += 64) d1[i] = s1[i];
    }
}
__device__ __forceinline__ void fill_row_bits(float *__restrict__ dst, int n, bool vec, int lane, unsigned bits) {
    if (vec) {
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int i = lane; i < n / 4; i += 64) d4[i] = make_uint4(bits, bits, bits, bits);
    } else {
        unsigned *d1 = reinterpret_cast<unsigned *>(dst);
        for (int i = lane; i < n; i += 64) d1[i] = bits;
    }
}
// copy_row_bits where a null source writes zeros (a function of its own: the select sits inside the loops)
__device__ __forceinline__ void copy_row_bits_or_zero(const float *__restrict__ src, float *__restrict__ dst, int n, bool vec, int lane) {
    if (vec) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int i = lane; i < n / 4; i += 64) d4[i] = src ? s4[i] : make_uint4(0u, 0u, 0u, 0u);
    } else {
        const unsigned *s1 = reinterpret_cast<const unsigned *>(src);
        unsigned *d1 = reinterpret_cast<unsigned *>(dst);
        for (int i = lane; i < n; i += 64) d1[i] = src ? s1[i] : 0u;
    }
}

// ---- band render: one workgroup renders the T steps of one image into one band of RB canvas rows (air_canvas_unroll_bands' banding,
// st_write_fwd_body's staging).  The LDS carve starts with the T bordered glimpses and the per-step axis tables; what a kernel keeps
// behind them (presence row, counters, reduction scratch) it lays out itself from `tail`.  The pieces below take tid and the number of
// threads and hold no barrier: the caller orders them and places the one barrier in front of its pixel loop.
struct BandCarve {
    float *glm, *tail;
    float2 *xe, *ye;                 // per (t, column) / (t, band row): {floor index as int bits | ST_INVALID, d}
    int hwp;
};
__device__ __forceinline__ BandCarve band_carve(float *smem, int T, int RB, int W, int h, int w) {
    BandCarve c;
    c.hwp = pad_count(h, w);
    float *p = smem;
    c.glm = p; p += (size_t)T * c.hwp;
    c.xe = reinterpret_cast<float2 *>(p); p += 2 * T * W;
    c.ye = reinterpret_cast<float2 *>(p); p += 2 * T * RB;
    c.tail = p;
    return c;
}
static inline size_t band_carve_floats(int T, int RB, int W, int h, int w) {      // the floats in front of `tail`
    return (size_t)T * pad_count_host(h, w) + 2 * (size_t)T * (W + RB);
}
// observation p of the band, requested ahead of its use: an unconditional load from a clamped address (no branch)
__device__ __forceinline__ float band_prefetch_obs(const float *ob, int ob_last, int p) { return ob[p < ob_last ? p : ob_last]; }
// the zero borders of the T bordered glimpses (the glimpse copy never overwrites them)
__device__ __forceinline__ void band_zero_borders(const BandCarve &c, int T, int h, int w, int tid, int nt) {
    for (int e = tid; e < T * pad_border(h, w); e += nt) {
        const int t = e / pad_border(h, w);
        c.glm[(size_t)t * c.hwp + pad_border_index(e - t * pad_border(h, w), h, w)] = 0.f;
    }
}
// glimpse[t, b] -> the interior of bordered glimpse t; vec4: w % 4 == 0 (a 16-byte group never straddles a glimpse row), aligned base
__device__ __forceinline__ void band_stage_glimpses(const BandCarve &c, const float *glimpse, bool vec4, int T, int B, int b,
                                                    int h, int w, int tid, int nt) {
    const int hw = h * w;
    const float inv_w = 1.0f / (float)w;
    if (vec4) {
        const int nq = hw >> 2;
        for (int e = tid; e < T * nq; e += nt) {
            const int t = e / nq, q = e - t * nq;
            const float4 v = reinterpret_cast<const float4 *>(glimpse + ((size_t)t * B + b) * hw)[q];
            float *d = c.glm + (size_t)t * c.hwp + pad_index(4 * q, w, inv_w);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        for (int e = tid; e < T * hw; e += nt) {
            const int t = e / hw, q = e - t * hw;
            c.glm[(size_t)t * c.hwp + pad_index(q, w, inv_w)] = glimpse[((size_t)t * B + b) * hw + q];
        }
    }
}
// the axis entries of where[t, b] = [sx, tx, sy, ty]: all W columns and the band's rows r0 .. r0 + nrow - 1 of every step
__device__ __forceinline__ void band_axis_tables(const BandCarve &c, const float *where, int T, int B, int b, int RB, int H,
                                                 int W, int h, int w, int r0, int nrow, double stepX, double stepY, int tid, int nt) {
#pragma clang fp contract(off)
    const float cxs = (float)((w - 1) / 2.0), cys = (float)((h - 1) / 2.0);
    for (int k = tid; k < T * (W + nrow); k += nt) {
        const int t = k / (W + nrow), r = k - t * (W + nrow);
        const float4 wk = *reinterpret_cast<const float4 *>(where + 4 * ((size_t)t * B + b));
        if (r < W) {
            c.xe[t * W + r] = axis_entry2(grid_coord(1.0f / wk.x, lin_m11(r, W, stepX), -wk.y / wk.x, cxs), w);
        } else {
            const int i = r - W;
            c.ye[t * RB + i] = axis_entry2(grid_coord(1.0f / wk.z, lin_m11(r0 + i, H, stepY), -wk.w / wk.z, cys), h);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
extern "C" int air_canvas_unroll_bands(int B, int H);
// What the banded launches behind a parse (air_prune_score, air_propose_residual) check once their own arguments are known to be
// present and in range: the caller sized its band shares for exactly air_canvas_unroll_bands(R, H) bands, `bits` (the addresses that
// only need 4-byte alignment, OR-ed) and `where`, and an LDS carve of the common head plus tail_floats that fits.
static inline int band_launch_prepare(int T, int R, int H, int W, int h, int w, int n_bands, const float *where, uintptr_t bits,
                                      size_t tail_floats, int *NB, int *RB, size_t *lds) {
    AIR_REQUIRE(n_bands == air_canvas_unroll_bands(R, H), AIR_E_SHAPE);
    AIR_REQUIRE((long)R * n_bands <= (long)INT_MAX && (long)H * W <= (long)INT_MAX / 2, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where), AIR_E_ALIGN);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    wr_bands(H, n_bands, NB, RB);
    AIR_REQUIRE(*NB == n_bands, AIR_E_SHAPE);
    *lds = sizeof(float) * (band_carve_floats(T, *RB, W, h, w) + tail_floats);
    AIR_REQUIRE(*lds <= CV_MAX_LDS, AIR_E_UNSUPPORTED);
    return AIR_OK;
}
// The relabel behind air_parse_objects, which labels rows by position (parse_kernels.hip): for j < num_objects[r] clipped to 0..T,
// score[j, r] = obj_score[offsets[r] + j] = score_src[j, r] and obj_step[offsets[r] + j] = ids[j, r].  air_prune_relabel and
// air_tile_relabel check their own arguments and launch it.
__attribute__((visibility("hidden"))) int parse_relabel_launch(const float *score_src, const int *ids, const int *num_objects,
                                                               const int *offsets, int T, int R, float *score, float *obj_score,
                                                               int *obj_step, void *stream);
