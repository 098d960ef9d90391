// Maximum-likelihood calibration of the trajectory smoother's noise terms for gfx950: the prediction-error decomposition of the
// constant-rate Kalman filter air_track_smooth runs, on a grid of G noise candidates in one pass over the tracker's tables.
//   air_track_noise_stats:  one workgroup of one wavefront per (sequence, candidate), one lane per track id (in passes of 64 ids); the
//                           forward filter alone at r = 1, q = the candidate's ratio, velocity_var = velocity_ratio; per noise class
//                           Q = sum e^2 / s~ and the product of the s~ as a normalised (mantissa, exponent) pair;
//   air_track_noise_reduce: the sequences combined in ascending order into device-resident totals (written or accumulated).
// The arithmetic is float64 from the widened fp32 values with contraction off, only + - * / and frexp, in the order and the combine
// order include/air_hip.h states; no workspace, no LDS, no floating-point atomics: the same bits run to run.
#include <limits.h>
#include <math.h>
#include "air_common.h"

#define NFIT_THREADS 64                  // one wavefront: a dependent chain per lane, the combine over the lanes by shuffles
#define NFIT_MAXT 32                     // TRACK_MAXT: objects per frame
#define NFIT_MAX_IDS 32767               // TRACK_MAX_IDS
#define NFIT_MAX_G 32                    // candidates per launch; air_track_noise_reduce has one lane per (candidate, class)
// the fit's domain: the smoother's supported ratios (csrc/trajectory_kernels.hip: TRAJ_Q_OVER_R_MIN, TRAJ_Q_OVER_R_MAX,
// TRAJ_V_OVER_R_MAX; trajectory.py asserts the equality), so that whatever is fitted is a setting the smoother takes
#define NFIT_Q_OVER_R_MIN 1e-29
#define NFIT_Q_OVER_R_MAX 1e15
#define NFIT_V_OVER_R_MAX 1e6

struct NoiseStatsArgs {
    const float *where;
    const int *num_objects, *track_id, *num_tracks, *track_first, *track_last;
    double *q, *m;
    int *k, *n;
    double ratio[2][NFIT_MAX_G];         // [0]: the shift components tx, ty; [1]: the scale components sx, sy
    double velocity_ratio;
    int T, S, F, G;
};

struct NfitCov {
    double xx, xv, vv;
};

// a product kept as m 2^k with m in [0.5, 1): (m, k) times (ms, ks)
__device__ __forceinline__ void nfit_mul(double &m, int &k, double ms, int ks) {
#pragma clang fp contract(off)
    int j;
    m = frexp(m * ms, &j);
    k += ks + j;
}

__device__ __forceinline__ void nfit_mul64(double &m, long long &k, double ms, long long ks) {
#pragma clang fp contract(off)
    int j;
    m = frexp(m * ms, &j);
    k += ks + (long long)j;
}

// One workgroup of one wavefront per (sequence s, candidate g), lane = track id (passes of 64 ids).  A track is taken iff
// 0 <= first <= last < F, as track_smooth_kernel takes it; the statements of the start, the predict and the update are that kernel's at
// r = 1.  An UPDATE is a frame after `first` with a sighting; the start and a coasted frame contribute nothing.
__global__ __launch_bounds__(NFIT_THREADS) void track_noise_stats_kernel(NoiseStatsArgs a) {
#pragma clang fp contract(off)
    const int T = a.T, F = a.F, R = a.S * F, FT = F * T;
    const int s = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    int issued = a.num_tracks[s];
    issued = issued < 0 ? 0 : (issued > FT ? FT : issued);
    const double q[2] = {a.ratio[0][g], a.ratio[1][g]};
    const double q2[2] = {0.5 * q[0], 0.5 * q[1]}, q4[2] = {0.25 * q[0], 0.25 * q[1]};
    double Qs[2] = {0.0, 0.0}, Ms[2] = {0.5, 0.5};                 // the sequence's, valid in lane 0
    int Ks[2] = {1, 1}, Ns = 0;

    for (int base = 0; base < issued; base += NFIT_THREADS) {
        const int id = base + lane;
        int first = -1, last = -1;
        if (id < issued) {
            first = a.track_first[(size_t)s * FT + id];
            last = a.track_last[(size_t)s * FT + id];
        }
        const bool valid = first >= 0 && first <= last && last < F;
        double Qt[2] = {0.0, 0.0}, Mt[2] = {0.5, 0.5};             // an idle lane carries the identities
        int Kt[2] = {1, 1}, Nt = 0;
        if (valid) {
            double x[4] = {0.0, 0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
            NfitCov P[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
            for (int f = first; f <= last; ++f) {
                const int r = s * F + f;
                int n = a.num_objects[r];
                n = n < 0 ? 0 : (n > T ? T : n);
                int j = -1;
                for (int t = n - 1; t >= 0; --t)
                    if (a.track_id[(size_t)t * R + r] == id) j = t;    // the lowest slot that carries the id
                const bool seen = j >= 0;
                double z[4] = {0.0, 0.0, 0.0, 0.0};
                if (seen) {
                    const float4 w4 = reinterpret_cast<const float4 *>(a.where)[(size_t)j * R + r];
                    z[0] = (double)w4.x, z[1] = (double)w4.y, z[2] = (double)w4.z, z[3] = (double)w4.w;
                }
                if (f == first) {                                  // start: x = z, v = 0, P = (1, 0, velocity_ratio)
#pragma unroll
                    for (int c = 0; c < 4; ++c) x[c] = z[c], v[c] = 0.0;
                    P[0].xx = P[1].xx = 1.0;
                    P[0].xv = P[1].xv = 0.0;
                    P[0].vv = P[1].vv = a.velocity_ratio;
                    continue;
                }
                NfitCov Pp[2];
                double xp[4];
#pragma unroll
                for (int c = 0; c < 2; ++c) {                      // predict (traj_predict_cov)
                    const double pa = P[c].xx + P[c].xv, pb = P[c].xv + P[c].vv;
                    Pp[c].xx = (pa + pb) + q4[c];
                    Pp[c].xv = pb + q2[c];
                    Pp[c].vv = P[c].vv + q[c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) xp[c] = x[c] + v[c];
                if (!seen) {                                       // a coasted frame keeps the predicted state
#pragma unroll
                    for (int c = 0; c < 4; ++c) x[c] = xp[c];
                    P[0] = Pp[0];
                    P[1] = Pp[1];
                    continue;
                }
                double kx[2], kv[2], sn[2], e[4];
#pragma unroll
                for (int c = 0; c < 2; ++c) {                      // update (TRAJ_UPDATE at r = 1)
                    sn[c] = Pp[c].xx + 1.0;
                    kx[c] = Pp[c].xx / sn[c];
                    kv[c] = Pp[c].xv / sn[c];
                    P[c].xx = Pp[c].xx - kx[c] * Pp[c].xx;
                    P[c].xv = Pp[c].xv - kx[c] * Pp[c].xv;
                    P[c].vv = Pp[c].vv - kv[c] * Pp[c].xv;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int cl = (c & 1) ? 0 : 1;                // [sx, tx, sy, ty]: the odd components are shifts
                    e[c] = z[c] - xp[c];
                    x[c] = xp[c] + kx[cl] * e[c];
                    v[c] = v[c] + kv[cl] * e[c];
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {                      // class 0: components 1, 3; class 1: components 0, 2
                    const int ca = c == 0 ? 1 : 0, cb = ca + 2;
                    const double d = (e[ca] * e[ca] + e[cb] * e[cb]) / sn[c];
                    Qt[c] = Qt[c] + d;
                    int ks;
                    const double ms = frexp(sn[c], &ks);
                    nfit_mul(Mt[c], Kt[c], ms, ks);
                }
                ++Nt;
            }
        }
        // the lanes of the pass: a binary tree, strides 32 .. 1, lane i < stride takes lane i + stride (every lane runs the statements;
        // lane 0 ends with the pass's value)
#pragma unroll
        for (int stride = NFIT_THREADS / 2; stride >= 1; stride >>= 1) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double qo = __shfl_down(Qt[c], stride), mo = __shfl_down(Mt[c], stride);
                const int ko = __shfl_down(Kt[c], stride);
                Qt[c] = Qt[c] + qo;
                nfit_mul(Mt[c], Kt[c], mo, ko);
            }
            Nt += __shfl_down(Nt, stride);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {                              // the passes in ascending order
            Qs[c] = Qs[c] + Qt[c];
            nfit_mul(Ms[c], Ks[c], Mt[c], Kt[c]);
        }
        Ns += Nt;
    }
    if (lane == 0) {
        const size_t at = ((size_t)s * a.G + g) * 2;
        a.q[at] = Qs[0], a.q[at + 1] = Qs[1];
        a.m[at] = Ms[0], a.m[at + 1] = Ms[1];
        a.k[at] = Ks[0], a.k[at + 1] = Ks[1];
        if (g == 0) a.n[s] = Ns;
    }
}

// the ratios as the entries take them (host code; a NaN fails every comparison)
static int nfit_ratio_check(int G, const double *shift_ratios, const double *scale_ratios, double velocity_ratio) {
    AIR_REQUIRE(G >= 1 && G <= NFIT_MAX_G, AIR_E_SHAPE);
    for (int g = 0; g < G; ++g) {
        AIR_REQUIRE(shift_ratios[g] >= NFIT_Q_OVER_R_MIN && shift_ratios[g] <= NFIT_Q_OVER_R_MAX, AIR_E_SHAPE);
        AIR_REQUIRE(scale_ratios[g] >= NFIT_Q_OVER_R_MIN && scale_ratios[g] <= NFIT_Q_OVER_R_MAX, AIR_E_SHAPE);
    }
    AIR_REQUIRE(velocity_ratio >= 0.0 && velocity_ratio <= NFIT_V_OVER_R_MAX, AIR_E_SHAPE);
    return AIR_OK;
}

extern "C" int air_track_noise_stats(const float *where, const int *num_objects, const int *track_id, const int *num_tracks,
                                     const int *track_first, const int *track_last, int T, int S, int F, int R, int G,
                                     const double *shift_ratios, const double *scale_ratios, double velocity_ratio, double *q,
                                     double *m, int *k, int *n, void *stream) {
    AIR_REQUIRE(where && num_objects && track_id && num_tracks && track_first && track_last && shift_ratios && scale_ratios && q && m &&
                k && n, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= NFIT_MAXT && S > 0 && F > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= NFIT_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(nfit_ratio_check(G, shift_ratios, scale_ratios, velocity_ratio) == AIR_OK, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where), AIR_E_ALIGN);
    AIR_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(m)) & 7u) == 0, AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(num_tracks) | reinterpret_cast<uintptr_t>(track_first) |
                           reinterpret_cast<uintptr_t>(track_last) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(n);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    NoiseStatsArgs a;
    a.where = where, a.num_objects = num_objects, a.track_id = track_id, a.num_tracks = num_tracks;
    a.track_first = track_first, a.track_last = track_last;
    a.q = q, a.m = m, a.k = k, a.n = n;
    for (int g = 0; g < NFIT_MAX_G; ++g) {
        a.ratio[0][g] = g < G ? shift_ratios[g] : 1.0;
        a.ratio[1][g] = g < G ? scale_ratios[g] : 1.0;
    }
    a.velocity_ratio = velocity_ratio;
    a.T = T, a.S = S, a.F = F, a.G = G;
    hipLaunchKernelGGL(track_noise_stats_kernel, dim3((unsigned)S, (unsigned)G), dim3(NFIT_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// reduce
// ============================================================================================================
struct NoiseReduceArgs {
    const double *q, *m;
    const int *k, *n;
    double *tot_q, *tot_m;
    long long *tot_k, *tot_n;
    int S, G, accumulate;
};

// One workgroup of one wavefront, lane = (candidate, class); the sequences in ascending order, then into the totals.
__global__ __launch_bounds__(NFIT_THREADS) void track_noise_reduce_kernel(NoiseReduceArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, G2 = 2 * a.G;
    if (lane < G2) {
        double Q = 0.0, M = 0.5;
        long long K = 1;
        const double *__restrict__ qs = a.q, *__restrict__ ms = a.m;
        const int *__restrict__ ks = a.k;
#pragma unroll 8
        for (int s = 0; s < a.S; ++s) {                            // (unrolled: the loads of eight sequences ahead of the dependent chain)
            const size_t at = (size_t)s * G2 + lane;
            Q = Q + qs[at];
            nfit_mul64(M, K, ms[at], (long long)ks[at]);
        }
        if (a.accumulate) {
            double tq = a.tot_q[lane], tm = a.tot_m[lane];
            long long tk = a.tot_k[lane];
            tq = tq + Q;
            nfit_mul64(tm, tk, M, K);
            Q = tq, M = tm, K = tk;
        }
        a.tot_q[lane] = Q;
        a.tot_m[lane] = M;
        a.tot_k[lane] = K;
    }
    if (lane == 0) {
        long long N = a.accumulate ? a.tot_n[0] : 0;
        for (int s = 0; s < a.S; ++s) N += (long long)a.n[s];
        a.tot_n[0] = N;
    }
}

extern "C" int air_track_noise_reduce(const double *q, const double *m, const int *k, const int *n, int S, int G, int accumulate,
                                      double *tot_q, double *tot_m, long long *tot_k, long long *tot_n, void *stream) {
    AIR_REQUIRE(q && m && k && n && tot_q && tot_m && tot_k && tot_n, AIR_E_NULL);
    AIR_REQUIRE(S > 0 && G >= 1 && G <= NFIT_MAX_G && (accumulate == 0 || accumulate == 1), AIR_E_SHAPE);
    const uintptr_t bits8 = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(tot_q) |
                            reinterpret_cast<uintptr_t>(tot_m) | reinterpret_cast<uintptr_t>(tot_k) | reinterpret_cast<uintptr_t>(tot_n);
    AIR_REQUIRE((bits8 & 7u) == 0, AIR_E_ALIGN);
    AIR_REQUIRE(((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(n)) & 3u) == 0, AIR_E_ALIGN);
    NoiseReduceArgs a = {q, m, k, n, tot_q, tot_m, tot_k, tot_n, S, G, accumulate};
    hipLaunchKernelGGL(track_noise_reduce_kernel, dim3(1), dim3(NFIT_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
