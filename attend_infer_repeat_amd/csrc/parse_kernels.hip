// Scene parsing of AIR for gfx950: the read-out behind a forward pass AT THE MODE of the inference network (zero latent noise,
// every Bernoulli draw forced to succeed: what = what_loc, where = where_loc after the guard rule, all T steps computed and
// nothing masked upstream).  The LSTM never sees the samples, so presence_prob -- and with it q(n | x) -- depends on the image
// alone, and that one pass holds the posterior means of all T steps and the exact count posterior.
//
//   air_parse_objects: count, presences, scores, boxes, and the flat object table of a batch.
//     m_0 = 1 - p_1,  m_n = (prod_{i<=n} p_i)(1 - p_{n+1}),  m_T = prod_i p_i   in float64, in index order (prior.py:62-68, the
//     arithmetic of air_numsteps_fwd);  n^ = the SMALLEST n attaining max_n m_n (the division by sum m does not enter the
//     arg-max), or num_objects_in clipped to 0..T when that is given (the convention of air_prior_latents).
//     presence[t, r] = t < n^;  score[t, r] = sum_{n>t} q(n) (fp32, added from n = T down: the engine's step_w);
//     boxes[t, r] = (left, top, width, height) = evaluation.attention_box(where[t, r], W, H) in fp32;
//     count_prob[r] = (float) q(n^).  Table: offsets[R + 1] = exclusive scan of num_objects, object j of image r in row
//     offsets[r] + j (image-major, step order inside an image), capacity T * R rows, rows from offsets[R] on are not written.
//   air_parse_render: canvas = sum_{t present} st_write(glimpse_t, where_t) in step order (cell.py:159-165),
//     reconstruction = mult * canvas, the band's share of the reconstruction term of air_rec_loglik_fwd against obs,
//     owner[r, p] = the smallest present t attaining max_t mult * layer_t(p) if that maximum is > mask_threshold, else -1 (int8),
//     area[t, r] = number of pixels step t owns (int32, integer adds), optionally layers[t, r] = mult * layer_t (0 for absent steps).
//
// The render stages an image exactly as st_write_fwd_body (canvas_kernels.hip) does -- bordered glimpses and the per-step axis
// tables in LDS behind one barrier -- and forms the value of step t at a pixel and the running sum with that body's operations
// (st_device.h: axis_entry2, load_taps_pad, bilerp; air_common.h: grid_coord, lin_m11; contraction off), so its canvas is
// bit-identical to air_canvas_unroll_fwd's for the same presences.
#include <math.h>
#include "scene_device.h"

#define PARSE_MAXT 32

// ============================================================================================================
// objects
// ============================================================================================================
// One wavefront per image (row r); lane t owns step t (T <= 32), lane n <= T also keeps m_n.  Every lane walks the same
// float64 chain (the probabilities travel by shuffle: wave-uniform values), so count and arg-max are the same bits in all lanes.
__global__ __launch_bounds__(256) void parse_count_kernel(const float *__restrict__ prob, const int *__restrict__ n_in,
                                                          const float *__restrict__ where, int T, int R, float Hf, float Wf,
                                                          int *__restrict__ n_out, float *__restrict__ count_prob,
                                                          float *__restrict__ presence, float *__restrict__ score,
                                                          float *__restrict__ boxes) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    int n_hat = 0;
    float q32 = __builtin_nanf(""), sc = __builtin_nanf("");      // no posterior given: score and count_prob are NaN
    if (prob) {
        const double p = lane < T ? (double)prob[(size_t)lane * R + r] : 0.0;
        double cum = 1.0, S = 0.0, best = 0.0, mine = 0.0;
        for (int n = 0; n <= T; ++n) {
            const double pn = __shfl(p, n < T ? n : 0, 64);
            const double m = n < T ? (1.0 - pn) * cum : cum;
            cum *= pn;
            S += m;
            if (n == 0 || m > best) { best = m; n_hat = n; }       // strict: the smallest n attaining the maximum
            if (lane == n) mine = m;
        }
        q32 = (float)(mine / S);                                   // q(n) in lane n <= T
        float w = 0.f;
        for (int t = T - 1; t >= 0; --t) {                         // step_w of air_numsteps_fwd: added from n = T down, in fp32
            w += __shfl(q32, t + 1, 64);
            if (lane == t) sc = w;
        }
    }
    if (n_in) {
        const int n = n_in[r];
        n_hat = n < 0 ? 0 : (n > T ? T : n);
    }
    const float qn = __shfl(q32, n_hat, 64);
    if (lane == 0) {
        n_out[r] = n_hat;
        count_prob[r] = qn;
    }
    if (lane < T) {
        const size_t k = (size_t)lane * R + r;
        presence[k] = lane < n_hat ? 1.f : 0.f;
        score[k] = sc;
        const float4 w4 = *reinterpret_cast<const float4 *>(where + 4 * k);      // [sx, tx, sy, ty]
        *reinterpret_cast<float4 *>(boxes + 4 * k) = attention_box4(w4, Wf, Hf);   // evaluation.attention_box, operation by operation
    }
}

// Exclusive scan of num_objects[R] by ONE workgroup, R in passes of 1024: inclusive scan inside each wave (shuffles), the
// sixteen wave totals through LDS, the running base carried from pass to pass.  Integers, one fixed order, no atomics.
__global__ __launch_bounds__(1024) void parse_scan_kernel(const int *__restrict__ n, int R, int *__restrict__ offsets) {
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int base = 0;
    for (int r0 = 0; r0 < R; r0 += 1024) {
        const int r = r0 + tid;
        const int v = r < R ? n[r] : 0;
        int inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (lane == 63) wave_tot[wid] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int wt = wave_tot[k];
            before += k < wid ? wt : 0;
            total += wt;
        }
        if (r < R) offsets[r] = base + before + inc - v;
        base += total;
        __syncthreads();                                           // wave_tot is rewritten by the next pass
    }
    if (tid == 0) offsets[R] = base;
}

// One wavefront per image copies its n^ rows into the table: lane j < n^ writes the row's scalars and its two float4, the A-wide
// `what` rows are spread over the lanes as n^ * A / V vectors of V floats (V = 4 / 2 / 1: what A and the row starts allow).
template <int V>
__global__ __launch_bounds__(256) void parse_scatter_kernel(const int *__restrict__ n_obj, const int *__restrict__ offsets,
                                                            const float *__restrict__ boxes, const float *__restrict__ score,
                                                            const float *__restrict__ where, const float *__restrict__ what,
                                                            int R, int A, int *__restrict__ obj_image, int *__restrict__ obj_step,
                                                            float *__restrict__ obj_box, float *__restrict__ obj_score,
                                                            float *__restrict__ obj_where, float *__restrict__ obj_what) {
    typedef typename VecOf<V>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    const int n = n_obj[r];
    const size_t row0 = (size_t)offsets[r];
    if (lane < n) {
        const size_t src = (size_t)lane * R + r, dst = row0 + lane;
        obj_image[dst] = r;
        obj_step[dst] = lane;
        obj_score[dst] = score[src];
        *reinterpret_cast<float4 *>(obj_box + 4 * dst) = *reinterpret_cast<const float4 *>(boxes + 4 * src);
        *reinterpret_cast<float4 *>(obj_where + 4 * dst) = *reinterpret_cast<const float4 *>(where + 4 * src);
    }
    const int AV = A / V, items = n * AV;
    for (int j = lane; j < items; j += 64) {
        const int t = j / AV, i = j - t * AV;
        *reinterpret_cast<vec_t *>(obj_what + (row0 + t) * A + (size_t)i * V) =
            *reinterpret_cast<const vec_t *>(what + ((size_t)t * R + r) * A + (size_t)i * V);
    }
}

extern "C" int air_parse_objects(const float *presence_prob, const int *num_objects_in, const float *where, const float *what,
                                 int T, int R, int A, int H, int W, int *num_objects, float *count_prob, float *presence,
                                 float *score, float *boxes, int *offsets, int *obj_image, int *obj_step, float *obj_box,
                                 float *obj_score, float *obj_where, float *obj_what, void *stream) {
    AIR_REQUIRE(where && what && num_objects && count_prob && presence && score && boxes && offsets && obj_image && obj_step &&
                obj_box && obj_score && obj_where && obj_what, AIR_E_NULL);
    AIR_REQUIRE(presence_prob || num_objects_in, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= PARSE_MAXT && R > 0 && A > 0 && H > 0 && W > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)T * R <= (long)INT_MAX, AIR_E_SHAPE);       // the table's row indices are int32
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(boxes) && air_aligned16(obj_box) && air_aligned16(obj_where), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(obj_what);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const dim3 grid(air_cdiv(R, 4)), block(256);
    hipLaunchKernelGGL(parse_count_kernel, grid, block, 0, air_stream(stream), presence_prob, num_objects_in, where, T, R, (float)H,
                       (float)W, num_objects, count_prob, presence, score, boxes);
    AIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(parse_scan_kernel, dim3(1), dim3(1024), 0, air_stream(stream), num_objects, R, offsets);
    AIR_LAUNCH_CHECK();
#define PARSE_LAUNCH(V)                                                                                                          \
    hipLaunchKernelGGL(parse_scatter_kernel<V>, grid, block, 0, air_stream(stream), num_objects, offsets, boxes, score, where, what, \
                       R, A, obj_image, obj_step, obj_box, obj_score, obj_where, obj_what)
    if (A % 4 == 0 && (bits & 15u) == 0) PARSE_LAUNCH(4);
    else if (A % 2 == 0 && (bits & 7u) == 0) PARSE_LAUNCH(2);
    else PARSE_LAUNCH(1);
#undef PARSE_LAUNCH
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// render
// ============================================================================================================
// behind the common head of the carve: the presence row, the pixels owned per step in this workgroup's band, block_sum's scratch
#define PARSE_TAIL_FLOATS (2 * PARSE_MAXT + 32)
struct ParseRenderArgs {
    const float *glimpse, *where, *presence, *obs;
    float *reconstruction, *rec_parts, *layers;
    signed char *owner;
    int *area;
    int T, B, NB, RB, H, W, h, w;
    double stepX, stepY;
    float mult, std, thr;
    int vec4_glimpse;
};
// One workgroup per (image, row band), air_canvas_unroll_bands' banding, st_write_fwd_body's staging: every global operand is
// requested up front, ONE barrier, then each thread walks its pixels (p = tid, tid + nt, ...: a wave's 64 pixels are adjacent) with
// the running canvas, the running maximum and its step in registers, t inner and in order.  The pixel loop has a wave-uniform trip
// count, so the pixels a step owns are counted with one ballot per step (lane t of every wave keeps the count of step t), folded
// through LDS and added to area[] once per workgroup and step.  Four adjacent lanes pack their owner bytes into one 32-bit store
// where the image's byte offset allows.
__global__ __launch_bounds__(1024) void parse_render_kernel(ParseRenderArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float smem[];
    const float *__restrict__ glimpse = a.glimpse, *__restrict__ where = a.where, *__restrict__ presence = a.presence;
    const float *__restrict__ obs = a.obs;
    float *__restrict__ recon = a.reconstruction, *__restrict__ rec_parts = a.rec_parts, *__restrict__ layers = a.layers;
    signed char *__restrict__ owner = a.owner;
    const int T = a.T, B = a.B, NB = a.NB, RB = a.RB, H = a.H, W = a.W, h = a.h, w = a.w;
    const float mult = a.mult, std = a.std, thr = a.thr;
    const int HW = H * W, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const BandCarve c = band_carve(smem, T, RB, W, h, w);
    float *pres = c.tail, *scratch = c.tail + 2 * PARSE_MAXT;
    int *cnt = reinterpret_cast<int *>(c.tail + PARSE_MAXT);
    const float cst = 0.5f * logf(6.283185307179586f) + logf(std);
    const int n_units = B * NB;
    const int pitch = w + 2;
    const float inv_W = 1.0f / (float)W;
    const bool owner_al4 = (reinterpret_cast<uintptr_t>(owner) & 3u) == 0;
    AIR_TR_INIT();
    band_zero_borders(c, T, h, w, tid, nt);                        // written once (visible after the first barrier below)
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int b = unit % B, band = unit / B;
        const int r0 = band * RB, r1 = (r0 + RB < H) ? r0 + RB : H, npx = (r1 - r0) * W, pbase = r0 * W;
        const size_t gbase = (size_t)b * HW + pbase;
        AIR_TR(0);
        // ---- every global load of this unit ------------------------------------------------------------------------------
        const float *ob = rec_parts ? obs + gbase : where;              // (any valid address when rec is not wanted)
        const int ob_last = rec_parts ? npx - 1 : 0;
        float xo[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xo[u] = band_prefetch_obs(ob, ob_last, tid + u * nt);
        if (unit != (int)blockIdx.x) __syncthreads();              // grid-stride reuse of the carve
        band_stage_glimpses(c, glimpse, a.vec4_glimpse != 0, T, B, b, h, w, tid, nt);
        band_axis_tables(c, where, T, B, b, RB, H, W, h, w, r0, r1 - r0, a.stepX, a.stepY, tid, nt);
        if (tid < T) {
            pres[tid] = presence[(size_t)tid * B + b];
            cnt[tid] = 0;
        }
        AIR_TR(1);
        __syncthreads();
        AIR_TR(2);
        const bool pack_ok = owner_al4 && (gbase & 3u) == 0;       // wave-uniform: quads of adjacent lanes start on a 4-byte boundary
        unsigned pmask = 0u;                                       // present steps, wave-uniform: read once per unit, not per pixel
        for (int t = 0; t < T; ++t) pmask |= (pres[t] > 0.5f ? 1u : 0u) << t;
        float s[1] = {0.f};
        int mine = 0;                                              // lane t: pixels step t owns among this wave's
        for (int base = 0; base < npx; base += 4 * nt) {           // (uniform trip count: ballots and shuffles inside)
            float xn[4] = {0.f, 0.f, 0.f, 0.f};
            if (base + 4 * nt < npx) {                             // next chunk's observations (bands above 4 pixels per thread)
#pragma unroll
                for (int u = 0; u < 4; ++u) xn[u] = band_prefetch_obs(ob, ob_last, base + tid + (4 + u) * nt);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = base + tid + u * nt;
                if (base + u * nt >= npx) break;                   // (uniform)
                const bool live = p < npx;
                int own = -1;
                if (live) {
                    const int Ib = div_small(p, W, inv_W), J = p - Ib * W;
                    float acc = 0.f, top = -INFINITY;
                    for (int t = 0; t < T; ++t) {
                        const bool present = (pmask >> t) & 1u;
                        float m = 0.f;
                        if (present) {
                            const float2 ex = c.xe[t * W + J], ey = c.ye[t * RB + Ib];
                            const int fx = __float_as_int(ex.x), fy = __float_as_int(ey.x);
                            float v = 0.f;
                            if (fx != ST_INVALID && fy != ST_INVALID)
                                v = bilerp(load_taps_pad(c.glm + (size_t)t * c.hwp, pitch, fy, fx), ex.y, ey.y);
                            acc = acc + v;                         // (== acc + 1.0f * v of the canvas write, bit for bit)
                            m = mult * v;
                            if (m > top) { top = m; own = t; }     // strict: the smallest step attaining the maximum
                        }
                        if (layers) layers[((size_t)t * B + b) * HW + pbase + p] = m;
                    }
                    if (!(top > thr)) own = -1;
                    const float rc = mult * acc;
                    recon[gbase + p] = rc;
                    if (rec_parts) {
                        const float z = (xo[u] - rc) / std;
                        s[0] += 0.5f * z * z + cst;
                    }
                }
                for (int t = 0; t < T; ++t) {
                    const int k = __popcll(__ballot(own == t));
                    if (lane == t) mine += k;
                }
                // owner bytes: lanes 4i .. 4i+3 hold adjacent pixels
                // (quad_perm DPP moves: lane 1 / 2 / 3 of every quad broadcast to the quad, one vector instruction each)
                const int ob8 = own & 0xff;
                const unsigned b1 = (unsigned)__builtin_amdgcn_mov_dpp(ob8, 0x55, 0xf, 0xf, true);
                const unsigned b2 = (unsigned)__builtin_amdgcn_mov_dpp(ob8, 0xaa, 0xf, 0xf, true);
                const unsigned b3 = (unsigned)__builtin_amdgcn_mov_dpp(ob8, 0xff, 0xf, 0xf, true);
                if (pack_ok && (p | 3) < npx) {
                    if ((lane & 3) == 0)
                        *reinterpret_cast<unsigned *>(owner + gbase + p) = (unsigned)ob8 | (b1 << 8) | (b2 << 16) | (b3 << 24);
                } else if (live) {
                    owner[gbase + p] = (signed char)own;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) xo[u] = xn[u];
        }
        AIR_TR(3);
        if (lane < T && mine) atomicAdd(&cnt[lane], mine);       // LDS, integers: the order does not matter
        if (rec_parts) {
            block_sum<1>(s, scratch);                              // (its barrier also covers the counts)
            if (tid == 0) rec_parts[(size_t)band * B + b] = s[0];
        } else {
            __syncthreads();
        }
        if (tid < T) {
            const int k = cnt[tid];
            if (k) atomicAdd(&a.area[(size_t)tid * B + b], k);
        }
        AIR_TR(4);
    }
    AIR_TR_FLUSH();
}

// WHICH form air_parse_render runs (bands, workgroup size, LDS, glimpse staging, grid): the decision the launch below consumes and
// air_parse_render_form returns -- no launch, no device memory touched; the status is the one the launch returns before its memset.
static int parse_render_form(const float *glimpse, const float *where, const float *presence, const float *obs,
                             const float *reconstruction, const float *rec_parts, const signed char *owner, const int *area, int T, int R,
                             int H, int W, int h, int w, int n_bands, AirWarpForm &f) {
    f = AirWarpForm{};
    AIR_REQUIRE(glimpse && where && presence && reconstruction && owner && area, AIR_E_NULL);
    AIR_REQUIRE(!rec_parts || obs, AIR_E_NULL);
    AIR_REQUIRE(T > 0 && T <= PARSE_MAXT && R > 0 && H > 0 && W > 0 && h > 0 && w > 0 && n_bands > 0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where), AIR_E_ALIGN);
    int NB, RB;
    wr_bands(H, n_bands, &NB, &RB);
    AIR_REQUIRE(NB == n_bands || !rec_parts, AIR_E_SHAPE);       // the caller sized rec_parts for exactly n_bands shares
    const size_t lds = sizeof(float) * (band_carve_floats(T, RB, W, h, w) + PARSE_TAIL_FLOATS);
    AIR_REQUIRE(lds <= CV_MAX_LDS, AIR_E_UNSUPPORTED);
    // workgroup sizes of the canvas write (launch_write_fwd): one pixel per thread while the launch is far from filling the chip
    const long units = (long)R * NB;
    int threads = units <= 512 ? 512 : ST_THREADS;
    if (units <= 256) {
        const int px = RB * W;
        threads = px >= 1024 ? 1024 : ((px + 63) / 64) * 64;
    }
    f.kernel = AIR_WARP_PARSE_RENDER;
    f.threads = threads; f.lds_bytes = (int)lds;
    f.vec4_glimpse = (w % 4 == 0) && air_aligned16(glimpse);
    f.NB = NB; f.RB = RB;
    f.items = units > (long)INT_MAX ? INT_MAX : (int)units; f.fixed_cap = 256 * 8; f.resident_cap = units > 256 * 8;
    return AIR_OK;
}
extern "C" int air_parse_render_form(const float *glimpse, const float *where, const float *presence, const float *obs,
                                     const float *reconstruction, const float *rec_parts, const signed char *owner, const int *area,
                                     int T, int R, int H, int W, int h, int w, int n_bands, AirWarpForm *out) {
    AIR_REQUIRE(out, AIR_E_NULL);
    return parse_render_form(glimpse, where, presence, obs, reconstruction, rec_parts, owner, area, T, R, H, W, h, w, n_bands, *out);
}

extern "C" int air_parse_render(const float *glimpse, const float *where, const float *presence, const float *obs, float mult,
                                float std, float mask_threshold, int T, int R, int H, int W, int h, int w, int n_bands,
                                float *reconstruction, float *rec_parts, signed char *owner, int *area, float *layers,
                                void *stream) {
    AirWarpForm f;
    int st = parse_render_form(glimpse, where, presence, obs, reconstruction, rec_parts, owner, area, T, R, H, W, h, w, n_bands, f);
    if (st) return st;
    const size_t lds = (size_t)f.lds_bytes;
    { int st_ = cv_allow_lds(parse_render_kernel, lds); if (st_) return st_; }
    hipError_t e = hipMemsetAsync(area, 0, sizeof(int) * (size_t)T * R, air_stream(stream));
    if (e != hipSuccess) return (int)e;
    const ParseRenderArgs a = {glimpse, where, presence, obs, reconstruction, rec_parts, layers, owner, area, T, R, f.NB, f.RB, H, W, h, w,
                               lin_step(W), lin_step(H), mult, std, mask_threshold, f.vec4_glimpse};
    const int cap = f.resident_cap ? air_resident_grid(parse_render_kernel, f.threads, lds, f.fixed_cap) : f.fixed_cap;
    hipLaunchKernelGGL(parse_render_kernel, dim3((unsigned)(f.items < cap ? f.items : cap)), dim3(f.threads), lds, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// relabel
// ============================================================================================================
// One wavefront per image; lane j < n rewrites what air_parse_objects labelled by position (scene_device.h states the rule).
__global__ __launch_bounds__(256) void parse_relabel_kernel(const float *__restrict__ score_src, const int *__restrict__ ids,
                                                            const int *__restrict__ n_obj, const int *__restrict__ offsets, int T,
                                                            int R, float *__restrict__ score, float *__restrict__ obj_score,
                                                            int *__restrict__ obj_step) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // wave-uniform
    int n = n_obj[r];
    n = n < 0 ? 0 : (n > T ? T : n);
    if (lane < n) {
        const size_t src = (size_t)lane * R + r, dst = (size_t)offsets[r] + lane;
        const float v = score_src[src];
        score[src] = v;
        obj_score[dst] = v;
        obj_step[dst] = ids[src];
    }
}

int parse_relabel_launch(const float *score_src, const int *ids, const int *num_objects, const int *offsets, int T, int R,
                         float *score, float *obj_score, int *obj_step, void *stream) {
    hipLaunchKernelGGL(parse_relabel_kernel, dim3(air_cdiv(R, 4)), dim3(256), 0, air_stream(stream), score_src, ids, num_objects,
                       offsets, T, R, score, obj_score, obj_step);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
