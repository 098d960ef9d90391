// Scoring a scene parse against ground truth for gfx950: detection (greedy box matching per IoU threshold) and segmentation
// (foreground ARI, best mask overlap) figures of a batch, computed where the parse lives.
//
//   air_score_contingency: cont[r, a, b] = #pixels of image r with owner + 1 == a and gt + 1 == b (int8 maps in, int32 counts out).
//   air_score_match:       per image, from cont and the two box lists: box IoU and mask IoU of every (step, object) pair, the greedy
//                          assignment per threshold, foreground ARI, best overlap per ground-truth object, count error.
//   air_score_reduce:      the sums of a validation set over the batch, by ONE workgroup in one fixed order.
//
// Everything a float decides is float64 with contraction off; every sum over pixels is an integer sum (LDS integer adds commute:
// the order does not matter); no floating-point atomic anywhere, so a rerun gives the same bits.
#include <limits.h>
#include <math.h>
#include "scene_device.h"

#define SCORE_MAXT 32
#define SCORE_MAXG 8
#define SCORE_MAXK 16
#define SCORE_MAXBINS ((SCORE_MAXT + 1) * (SCORE_MAXG + 1))

// ============================================================================================================
// contingency
// ============================================================================================================
// bin of a pixel, or -1 when either label is outside its range (the parser's sentinel, a gt label past G): counted nowhere
__device__ __forceinline__ int score_bin(int o, int g, int T, int G) {
    const int a = o + 1, b = g + 1;
    return ((unsigned)a <= (unsigned)T && (unsigned)b <= (unsigned)G) ? a * (G + 1) + b : -1;
}
// A thread's pixels are adjacent, and neighbouring pixels mostly share their labels (background, the inside of a digit): a run of
// equal bins costs one LDS add when it ends, not one per pixel.
struct ScoreRun {
    int bin, len;
    __device__ __forceinline__ void push(int b, int *hist) {
        if (b == bin) { ++len; return; }
        if (bin >= 0) atomicAdd(&hist[bin], len);
        bin = b;
        len = 1;
    }
    __device__ __forceinline__ void flush(int *hist) {
        if (bin >= 0 && len) atomicAdd(&hist[bin], len);
        len = 0;
    }
};
__device__ __forceinline__ void score_push_word(ScoreRun &run, unsigned wo, unsigned wg, int T, int G, int *hist) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        run.push(score_bin((int)(signed char)(wo >> (8 * i)), (int)(signed char)(wg >> (8 * i)), T, G), hist);
}

// One workgroup per image (grid-stride over the images), one histogram of (T+1)(G+1) bins per wave in LDS, merged by integer adds
// behind one barrier; thread i < nbins writes bin i, so every bin of cont is written.  The body of an image is read as 16-byte
// vectors from the first 16-byte boundary of its owner row on (possible when the gt row has the same offset from a boundary: the
// two rows start r * H * W bytes into their buffers); the bytes in front of that boundary and behind the last whole vector -- and
// all of the image when the two rows disagree -- go one at a time, by the first threads.
__global__ __launch_bounds__(1024) void score_contingency_kernel(const signed char *__restrict__ owner,
                                                                 const signed char *__restrict__ gt, int T, int G, int R, int HW,
                                                                 int *__restrict__ cont) {
    extern __shared__ int hist_all[];                              // (waves) x (T+1)(G+1) bins: 144 bytes at 50x50 / T = 3 / G = 2, 19 KB at most
    const int tid = threadIdx.x, nt = blockDim.x, wid = tid >> 6, nw = nt >> 6;
    const int nbins = (T + 1) * (G + 1);
    int *hist = hist_all + wid * nbins;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        for (int i = tid; i < nw * nbins; i += nt) hist_all[i] = 0;
        __syncthreads();
        const signed char *po = owner + (size_t)r * HW, *pg = gt + (size_t)r * HW;
        const unsigned mo = (unsigned)(reinterpret_cast<uintptr_t>(po) & 15u), mg = (unsigned)(reinterpret_cast<uintptr_t>(pg) & 15u);
        int head = HW, nvec = 0;                                   // rows that disagree: every byte on the scalar path
        if (mo == mg) {
            head = (int)((16u - mo) & 15u);
            if (head > HW) head = HW;
            nvec = (HW - head) >> 4;
        }
        const int tail0 = head + 16 * nvec;                        // first byte behind the vectors
        ScoreRun run = {-1, 0};
        const uint4 *vo = reinterpret_cast<const uint4 *>(po + head), *vg = reinterpret_cast<const uint4 *>(pg + head);
        for (int v = tid; v < nvec; v += nt) {
            const uint4 a = vo[v], b = vg[v];
            score_push_word(run, a.x, b.x, T, G, hist);
            score_push_word(run, a.y, b.y, T, G, hist);
            score_push_word(run, a.z, b.z, T, G, hist);
            score_push_word(run, a.w, b.w, T, G, hist);
        }
        run.flush(hist);
        const int n_edge = head + (HW - tail0);                    // < 32 unless the rows disagree
        for (int e = tid; e < n_edge; e += nt) {
            const int p = e < head ? e : tail0 + (e - head);
            const int b = score_bin((int)po[p], (int)pg[p], T, G);
            if (b >= 0) atomicAdd(&hist[b], 1);
        }
        __syncthreads();
        for (int i = tid; i < nbins; i += nt) {
            int s = 0;
            for (int w = 0; w < nw; ++w) s += hist_all[w * nbins + i];
            cont[(size_t)r * nbins + i] = s;
        }
        __syncthreads();                                           // the histograms are zeroed again for the next image
    }
}

static inline bool score_dims_ok(int T, int G, int R) {
    return T >= 1 && T <= SCORE_MAXT && G >= 1 && G <= SCORE_MAXG && R > 0 && (long)R * (T + 1) * (G + 1) <= (long)INT_MAX;
}

extern "C" int air_score_contingency(const signed char *owner, const signed char *gt, int T, int G, int R, int H, int W, int *cont,
                                     void *stream) {
    AIR_REQUIRE(owner && gt && cont, AIR_E_NULL);
    AIR_REQUIRE(H > 0 && W > 0 && score_dims_ok(T, G, R), AIR_E_SHAPE);
    AIR_REQUIRE((long)R * H * W <= (long)INT_MAX && (long)H * W <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE((reinterpret_cast<uintptr_t>(cont) & 3u) == 0, AIR_E_ALIGN);
    const int HW = H * W;
    // one 16-byte vector per thread while the image is small: 2500 pixels are three waves, several such workgroups share a CU
    int threads = ((air_cdiv(HW, 16) + 63) / 64) * 64;
    threads = threads < 64 ? 64 : (threads > 1024 ? 1024 : threads);
    const int cap = 256 * 16;
    hipLaunchKernelGGL(score_contingency_kernel, dim3((unsigned)(R < cap ? R : cap)), dim3(threads),
                       sizeof(int) * (size_t)(threads / 64) * (T + 1) * (G + 1), air_stream(stream), owner, gt, T, G, R, HW, cont);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// match
// ============================================================================================================
__device__ __forceinline__ long long score_shfl_xor(long long v, int mask) {
    int lo = (int)(v & 0xffffffffll), hi = (int)(v >> 32);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return ((long long)hi << 32) | (long long)(unsigned)lo;
}
__device__ __forceinline__ long long score_wave_sum(long long v) {      // valid in every lane; integers: the order does not matter
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += score_shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ long long score_pairs(long long n) { return n * (n - 1) / 2; }

// One wavefront per image.  The image's contingency table and the float64 box IoUs of its T x G pairs live in the wave's slice of
// LDS; lane a <= T owns row a of the table, lane b <= G column b, lane k < K walks the greedy assignment of threshold k.
__global__ __launch_bounds__(256) void score_match_kernel(const int *__restrict__ cont, const float *__restrict__ boxes,
                                                          const int *__restrict__ num_objects, const float *__restrict__ gt_boxes,
                                                          const int *__restrict__ gt_count, const float *__restrict__ thresholds,
                                                          int T, int G, int K, int R, float *__restrict__ box_iou,
                                                          float *__restrict__ mask_iou, signed char *__restrict__ match,
                                                          float *__restrict__ ari, float *__restrict__ best_overlap,
                                                          int *__restrict__ count_err) {
#pragma clang fp contract(off)
    __shared__ int cont_s[4][SCORE_MAXBINS];
    __shared__ int rowsum_s[4][SCORE_MAXT + 1], colsum_s[4][SCORE_MAXG + 1];
    __shared__ double biou_s[4][SCORE_MAXT * SCORE_MAXG];
    __shared__ float miou_s[4][SCORE_MAXT * SCORE_MAXG];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wid;
    if (r >= R) return;                                            // wave-uniform; no workgroup barrier below
    const int G1 = G + 1, nbins = (T + 1) * G1;
    int *c = cont_s[wid];
    for (int i = lane; i < nbins; i += 64) c[i] = cont[(size_t)r * nbins + i];
    int nh = num_objects[r], g = gt_count[r];
    nh = nh < 0 ? 0 : (nh > T ? T : nh);
    g = g < 0 ? 0 : (g > G ? G : g);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- row and column sums; the foreground (b >= 1) pair counts --------------------------------------------------------------
    long long A_fg = 0, S_row = 0, B_col = 0;
    if (lane <= T) {
        int all = c[lane * G1];
        for (int b = 1; b <= G; ++b) {
            const long long n = c[lane * G1 + b];
            all += (int)n;
            A_fg += n;
            S_row += score_pairs(n);
        }
        rowsum_s[wid][lane] = all;                                 // a_t of the mask IoU counts every pixel the step owns
    }
    if (lane <= G) {
        for (int a = 0; a <= T; ++a) B_col += c[a * G1 + lane];
        colsum_s[wid][lane] = (int)B_col;
    }
    const long long N = score_wave_sum(A_fg), S = score_wave_sum(S_row), P = score_wave_sum(lane <= T ? score_pairs(A_fg) : 0ll);
    const long long Q = score_wave_sum(lane >= 1 && lane <= G ? score_pairs(B_col) : 0ll);
    if (lane == 0) {
        const long long C = score_pairs(N);
        float v;
        if (N == 0) v = __builtin_nanf("");
        else if (C == 0) v = 1.f;
        else {
            const double E = (double)P * (double)Q / (double)C, M = ((double)P + (double)Q) / 2.0;
            v = M == E ? 1.f : (float)(((double)S - E) / (M - E));
        }
        ari[r] = v;
        count_err[r] = nh - g;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- the T x G pairs ------------------------------------------------------------------------------------------------------
    for (int p = lane; p < T * G; p += 64) {
        const int t = p / G, j = p - t * G;
        double bi = 0.0, mi = 0.0;
        if (t < nh && j < g) {
            const float4 pb = *reinterpret_cast<const float4 *>(boxes + 4 * ((size_t)t * R + r));
            const float4 gb = *reinterpret_cast<const float4 *>(gt_boxes + 4 * ((size_t)r * G + j));
            bi = box_iou_f64(pb, gb);
            const long long n = c[(t + 1) * G1 + j + 1];
            const long long uni = (long long)rowsum_s[wid][t + 1] + (long long)colsum_s[wid][j + 1] - n;
            mi = uni > 0 ? (double)n / (double)uni : 0.0;
        }
        biou_s[wid][p] = bi;
        miou_s[wid][p] = (float)mi;
        box_iou[(size_t)r * T * G + p] = (float)bi;
        mask_iou[(size_t)r * T * G + p] = (float)mi;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- best overlap per ground-truth object (the maximum of the rounded values is the rounded maximum) ------------------------
    if (lane < G) {
        float best = lane < g ? 0.f : -1.f;
        if (lane < g)
            for (int t = 0; t < nh; ++t) best = fmaxf(best, miou_s[wid][t * G + lane]);
        best_overlap[(size_t)r * G + lane] = best;
    }
    // ---- greedy assignment, one threshold per lane -----------------------------------------------------------------------------
    if (lane < K) {
        const double tau = (double)thresholds[lane];
        unsigned used = 0u;
        for (int t = 0; t < T; ++t) {
            int pick = -1;
            if (t < nh) {
                double top = 0.0;
                for (int j = 0; j < g; ++j) {
                    const double v = biou_s[wid][t * G + j];
                    if (!((used >> j) & 1u) && v > 0.0 && v >= tau && v > top) { top = v; pick = j; }      // strict: smallest j on a tie
                }
                if (pick >= 0) used |= 1u << pick;
            }
            match[((size_t)lane * T + t) * R + r] = (signed char)pick;
        }
    }
}

extern "C" int air_score_match(const int *cont, const float *boxes, const int *num_objects, const float *gt_boxes,
                               const int *gt_count, const float *thresholds, int T, int G, int K, int R, float *box_iou,
                               float *mask_iou, signed char *match, float *ari, float *best_overlap, int *count_err, void *stream) {
    AIR_REQUIRE(cont && boxes && num_objects && gt_boxes && gt_count && thresholds && box_iou && mask_iou && match && ari &&
                best_overlap && count_err, AIR_E_NULL);
    AIR_REQUIRE(K >= 1 && K <= SCORE_MAXK && score_dims_ok(T, G, R), AIR_E_SHAPE);
    AIR_REQUIRE((long)R * T * (K > G ? K : G) <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(boxes) && air_aligned16(gt_boxes), AIR_E_ALIGN);
    hipLaunchKernelGGL(score_match_kernel, dim3(air_cdiv(R, 4)), dim3(256), 0, air_stream(stream), cont, boxes, num_objects, gt_boxes,
                       gt_count, thresholds, T, G, K, R, box_iou, mask_iou, match, ari, best_overlap, count_err);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// reduce
// ============================================================================================================
#define SCORE_NI (6 + SCORE_MAXK)
// ONE workgroup of 1024 threads.  Thread i adds the images i, i + 1024, i + 2048, ... in that order into its own partial sums
// (R in passes of 1024); the 64 partials of a wave are then added by the shuffle tree of wave_sum (offsets 32, 16, .., 1), and
// thread 0 adds the sixteen wave totals in wave order.  The order depends on R alone.  Inside an image the best overlaps are
// added in object order and the matched IoUs in step order.
__global__ __launch_bounds__(1024) void score_reduce_kernel(const int *__restrict__ num_objects, const int *__restrict__ gt_count,
                                                            const int *__restrict__ count_err, const float *__restrict__ ari,
                                                            const float *__restrict__ best_overlap,
                                                            const signed char *__restrict__ match,
                                                            const float *__restrict__ box_iou, int T, int G, int K, int R,
                                                            long long *__restrict__ totals_i, double *__restrict__ totals_f,
                                                            int accumulate) {
#pragma clang fp contract(off)
    __shared__ long long wi[16][SCORE_NI];
    __shared__ double wf[16][3];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    long long si[SCORE_NI];
    double sf[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < SCORE_NI; ++i) si[i] = 0;
    for (int r = tid; r < R; r += 1024) {
        int nh = num_objects[r], g = gt_count[r];
        nh = nh < 0 ? 0 : (nh > T ? T : nh);
        g = g < 0 ? 0 : (g > G ? G : g);
        const int ce = count_err[r];
        si[0] += 1;
        si[1] += ce == 0 ? 1 : 0;
        si[2] += ce < 0 ? -(long long)ce : (long long)ce;
        si[3] += nh;
        si[4] += g;
        const float a = ari[r];
        if (isfinite(a)) {
            si[5] += 1;
            sf[0] += (double)a;
        }
        for (int j = 0; j < g; ++j) sf[1] += (double)best_overlap[(size_t)r * G + j];
#pragma unroll
        for (int k = 0; k < SCORE_MAXK; ++k) {
            for (int t = 0; t < (k < K ? nh : 0); ++t) {
                const int j = match[((size_t)k * T + t) * R + r];
                if (j >= 0 && j < G) {
                    si[6 + k] += 1;
                    if (k == 0) sf[2] += (double)box_iou[((size_t)r * T + t) * G + j];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SCORE_NI; ++i) si[i] = score_wave_sum(si[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) sf[i] = wave_sum(sf[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < SCORE_NI; ++i) wi[wid][i] = si[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) wf[wid][i] = sf[i];
    }
    __syncthreads();
    if (tid < 6 + K) {
        long long s = 0;
        for (int w = 0; w < 16; ++w) s += wi[w][tid];
        totals_i[tid] = accumulate ? totals_i[tid] + s : s;
    } else if (tid >= 64 && tid < 67) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += wf[w][tid - 64];
        totals_f[tid - 64] = accumulate ? totals_f[tid - 64] + s : s;
    }
}

extern "C" int air_score_reduce(const int *num_objects, const int *gt_count, const int *count_err, const float *ari,
                                const float *best_overlap, const signed char *match, const float *box_iou, int T, int G, int K, int R,
                                int64_t *totals_i, double *totals_f, int accumulate, void *stream) {
    AIR_REQUIRE(num_objects && gt_count && count_err && ari && best_overlap && match && box_iou && totals_i && totals_f, AIR_E_NULL);
    AIR_REQUIRE(K >= 1 && K <= SCORE_MAXK && score_dims_ok(T, G, R), AIR_E_SHAPE);
    AIR_REQUIRE((long)R * T * (K > G ? K : G) <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(((reinterpret_cast<uintptr_t>(totals_i) | reinterpret_cast<uintptr_t>(totals_f)) & 7u) == 0, AIR_E_ALIGN);
    hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(1024), 0, air_stream(stream), num_objects, gt_count, count_err, ari,
                       best_overlap, match, box_iou, T, G, K, R, reinterpret_cast<long long *>(totals_i), totals_f, accumulate);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
