// Trajectories behind the sequence tracker for gfx950: smoothed, gap-filled and extrapolated tracks.
//   air_track_smooth: per sequence one workgroup, one lane per track id (in passes of 64 ids); a constant-rate Kalman
//                     filter forward over the track's span and a Rauch-Tung-Striebel pass (means only) back, per `where` component;
//                     the completed table (a row for every track that spans a frame, sighted there or not) and the forecast table;
//   air_track_fill:   what / glimpse / score of the completed or forecast rows: bit copies of the source sighting's rows.
// The arithmetic is float64 from the widened fp32 values with contraction off, only + - * /, in the order include/air_hip.h states;
// the row of a track in a frame is a count of integers in one fixed order; no floating-point atomics: the same bits run to run.
#include <limits.h>
#include "scene_device.h"
#include "traj_device.h"

#define TRAJ_THREADS 256                 // air_track_fill: four wavefronts, one (row, column) each
#define TRAJ_SMOOTH_THREADS 64           // air_track_smooth: one wavefront per sequence -- a dependent chain per lane, no cross-wave traffic
#define TRAJ_MAXT 32                     // TRACK_MAXT: objects per frame, live tracks per sequence, rows of the completed table
#define TRAJ_MAX_IDS 32767               // TRACK_MAX_IDS
#define TRAJ_MAX_HORIZON 16
// the supported noise domain (include/air_hip.h states it and where it was measured): outside it the call is refused
#define TRAJ_Q_OVER_R_MIN 1e-29          // q_shift / r and q_scale / r, both
#define TRAJ_Q_OVER_R_MAX 1e15
#define TRAJ_V_OVER_R_MAX 1e6            // velocity_var / r (0 is inside)
#define TRAJ_R_MIN 1e-146
#define TRAJ_R_MAX 1e134
#define TRAJ_WS_DOUBLES 28               // per (row, frame): 4 x (x, v, x-, v-), 2 noise classes x (P, P-) of three values each

enum { TRAJ_ABSENT = 0, TRAJ_OBSERVED = 1, TRAJ_FILLED = 2, TRAJ_FORECAST = 3 };
// workspace planes: plane k of row `row` in frame r is ws[((size_t)k * R + r) * C + row]
enum { WS_X = 0, WS_V = 4, WS_XP = 8, WS_VP = 12, WS_P = 16, WS_PP = 19 };      // class c: WS_P + 6 c, WS_PP + 6 c

struct TrajSmoothArgs {
    const float *where;
    const int *num_objects, *track_id, *num_tracks, *track_first, *track_last;
    double *ws;
    float *sm_where, *sm_boxes, *sm_velocity, *fc_where, *fc_boxes, *fc_velocity;
    int *sm_id, *sm_src_frame, *sm_src_slot, *sm_count, *sm_counts, *fc_id, *fc_src_frame, *fc_src_slot, *fc_count;
    signed char *sm_state, *fc_state;
    double q[2], r, velocity_var;        // q[0]: the shift components tx, ty; q[1]: the scale components sx, sy
    int T, S, F, C, Hz, max_age, H, W;
};

// The predict step and the update (TRAJ_UPDATE) are traj_device.h's: the tracker's motion state runs the same text.  The backward step
// is shared by track_smooth_kernel and the stream kernels as TEXT, like the update.
// back: (xs, vs) of frame f in place from those of frame f + 1; w: the planes of frame f, wn: of frame f + 1, `plane` apart
#define TRAJ_BACK(w, wn, plane, xs, vs)                                                                                       \
    {                                                                                                                         \
        double C00[2], C01[2], C10[2], C11[2];                                                                                \
        _Pragma("unroll") for (int c = 0; c < 2; ++c) {                                                                       \
            const double pxx = w[(WS_P + 6 * c) * plane], pxv = w[(WS_P + 6 * c + 1) * plane], pvv = w[(WS_P + 6 * c + 2) * plane]; \
            const double nxx = wn[(WS_PP + 6 * c) * plane], nxv = wn[(WS_PP + 6 * c + 1) * plane],                            \
                         nvv = wn[(WS_PP + 6 * c + 2) * plane];                                                               \
            const double g00 = pxx + pxv, g01 = pxv, g10 = pxv + pvv, g11 = pvv;                                              \
            const double det = nxx * nvv - nxv * nxv;                                                                         \
            C00[c] = (g00 * nvv - g01 * nxv) / det;                                                                           \
            C01[c] = (g01 * nxx - g00 * nxv) / det;                                                                           \
            C10[c] = (g10 * nvv - g11 * nxv) / det;                                                                           \
            C11[c] = (g11 * nxx - g10 * nxv) / det;                                                                           \
        }                                                                                                                     \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                                       \
            const int cl = (c & 1) ? 0 : 1;                                                                                   \
            const double dx = xs[c] - wn[(WS_XP + c) * plane], dv = vs[c] - wn[(WS_VP + c) * plane];                          \
            xs[c] = w[(WS_X + c) * plane] + (C00[cl] * dx + C01[cl] * dv);                                                    \
            vs[c] = w[(WS_V + c) * plane] + (C10[cl] * dx + C11[cl] * dv);                                                    \
        }                                                                                                                     \
    }

// the rule's arguments, one-shot and stream alike, and air_track_associate_motion's (host code; a NaN fails every comparison)
int traj_noise_check(double q_shift, double q_scale, double r, double velocity_var) {
    AIR_REQUIRE(q_shift > 0.0 && q_scale > 0.0 && r > 0.0 && velocity_var >= 0.0, AIR_E_SHAPE);
    AIR_REQUIRE(r >= TRAJ_R_MIN && r <= TRAJ_R_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(q_shift / r >= TRAJ_Q_OVER_R_MIN && q_shift / r <= TRAJ_Q_OVER_R_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(q_scale / r >= TRAJ_Q_OVER_R_MIN && q_scale / r <= TRAJ_Q_OVER_R_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(velocity_var / r <= TRAJ_V_OVER_R_MAX, AIR_E_SHAPE);
    return AIR_OK;
}

// Every output of the sequence starts ABSENT; the lanes of the spanning tracks overwrite their rows behind a barrier.
__device__ __forceinline__ void traj_fill_absent(const TrajSmoothArgs &a, int s, int tid) {
    const int F = a.F, C = a.C, Hz = a.Hz;
    const size_t R = (size_t)a.S * F, N = (size_t)a.S * Hz;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = tid; e < C * F; e += TRAJ_SMOOTH_THREADS) {
        const int c = e / F, f = e - c * F;
        const size_t at = (size_t)c * R + (size_t)s * F + f;
        reinterpret_cast<float4 *>(a.sm_where)[at] = z4;
        reinterpret_cast<float4 *>(a.sm_boxes)[at] = z4;
        a.sm_velocity[2 * at] = 0.f;
        a.sm_velocity[2 * at + 1] = 0.f;
        a.sm_id[at] = -1;
        a.sm_state[at] = (signed char)TRAJ_ABSENT;
        a.sm_src_frame[at] = -1;
        a.sm_src_slot[at] = -1;
    }
    for (int f = tid; f < F; f += TRAJ_SMOOTH_THREADS) a.sm_count[(size_t)s * F + f] = 0;
    for (int e = tid; e < C * Hz; e += TRAJ_SMOOTH_THREADS) {
        const int c = e / Hz, k = e - c * Hz;
        const size_t at = (size_t)c * N + (size_t)s * Hz + k;
        reinterpret_cast<float4 *>(a.fc_where)[at] = z4;
        reinterpret_cast<float4 *>(a.fc_boxes)[at] = z4;
        a.fc_velocity[2 * at] = 0.f;
        a.fc_velocity[2 * at + 1] = 0.f;
        a.fc_id[at] = -1;
        a.fc_state[at] = (signed char)TRAJ_ABSENT;
        a.fc_src_frame[at] = -1;
        a.fc_src_slot[at] = -1;
    }
    for (int k = tid; k < Hz; k += TRAJ_SMOOTH_THREADS) a.fc_count[(size_t)s * Hz + k] = 0;
}

// One workgroup of one wavefront per sequence, lane = track id (passes of 64 ids).  A track is taken iff 0 <= first <= last < F.  Ids are
// issued in frame order, so every id' < id was born no later than id: the ids below one's own that span a frame f >= first are
// among those with last' >= first -- at most 31 of them, since all of them and id itself span `first`.  Their `last` values are
// kept in LDS (olast_s[k][lane]); the row in frame f is the number of them with last' >= f.
__global__ __launch_bounds__(TRAJ_SMOOTH_THREADS) void track_smooth_kernel(TrajSmoothArgs a) {
#pragma clang fp contract(off)
    __shared__ int olast_s[TRAJ_MAXT][TRAJ_SMOOTH_THREADS];
    __shared__ int first_s[TRAJ_SMOOTH_THREADS], last_s[TRAJ_SMOOTH_THREADS];
    __shared__ int counts_s[2];
    const int T = a.T, F = a.F, C = a.C, Hz = a.Hz, R = a.S * F, FT = F * T;
    const int s = blockIdx.x, tid = threadIdx.x;
    const size_t N = (size_t)a.S * Hz;
    int issued = a.num_tracks[s];
    issued = issued < 0 ? 0 : (issued > FT ? FT : issued);
    const int live_from = F - 1 - a.max_age;                       // a track last seen in this frame or later is live after frame F - 1
    const double q2[2] = {0.5 * a.q[0], 0.5 * a.q[1]}, q4[2] = {0.25 * a.q[0], 0.25 * a.q[1]};
    const float Wf = (float)a.W, Hf = (float)a.H;
    if (tid < 2) counts_s[tid] = 0;
    traj_fill_absent(a, s, tid);
    __syncthreads();

    for (int base = 0; base < issued; base += TRAJ_SMOOTH_THREADS) {
        const int id = base + tid;
        int first = -1, last = -1;
        if (id < issued) {
            first = a.track_first[(size_t)s * FT + id];
            last = a.track_last[(size_t)s * FT + id];
        }
        const bool valid = first >= 0 && first <= last && last < F;
        const bool forecast = valid && Hz > 0 && last >= live_from;
        const int reach = forecast && live_from < first ? live_from : first;      // the ids below that matter have last' >= reach
        // ---- the ids below one's own that overlap: chunks of 64 (first, last) pairs through LDS, read by every lane in ascending id ----
        int m = 0;
        for (int cb = 0; cb <= base; cb += TRAJ_SMOOTH_THREADS) {
            __syncthreads();                                       // (the previous chunk, or the previous pass, is read)
            const int oid = cb + tid;
            int of = -1, ol = -1;
            if (oid < issued) {
                of = a.track_first[(size_t)s * FT + oid];
                ol = a.track_last[(size_t)s * FT + oid];
            }
            first_s[tid] = of;
            last_s[tid] = ol;
            __syncthreads();
            const int upto = id - cb < TRAJ_SMOOTH_THREADS ? id - cb : TRAJ_SMOOTH_THREADS;      // ids cb .. cb + upto - 1 are below one's own
            if (valid)
                for (int k = 0; k < upto; ++k) {
                    const int of2 = first_s[k], ol2 = last_s[k];
                    if (of2 >= 0 && of2 <= ol2 && ol2 < F && ol2 >= reach && m < TRAJ_MAXT) olast_s[m++][tid] = ol2;
                }
        }
        if (!valid) continue;                                      // (no barrier below this line inside the pass)

        // ---- forward: the filter over first .. last ------------------------------------------------------------------------------------------
        double x[4] = {0.0, 0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
        TrajCov P[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        int src_f = -1, src_j = -1, n_obs = 0, n_fill = 0;
        for (int f = first; f <= last; ++f) {
            const int r = s * F + f;
            int row = 0;
            for (int k = 0; k < m; ++k) row += olast_s[k][tid] >= f ? 1 : 0;
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
                src_f = f;
                src_j = j;
            }
            TrajCov Pp[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
            double xp[4] = {0.0, 0.0, 0.0, 0.0}, vp[4] = {0.0, 0.0, 0.0, 0.0};
            if (f == first) {                                      // start: x = z, v = 0, P = (r, 0, velocity_var)
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c] = z[c], v[c] = 0.0;
                P[0].xx = P[1].xx = a.r;
                P[0].xv = P[1].xv = 0.0;
                P[0].vv = P[1].vv = a.velocity_var;
            } else {
#pragma unroll
                for (int c = 0; c < 2; ++c) Pp[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) xp[c] = x[c] + v[c], vp[c] = v[c];
                if (seen) {
                    TRAJ_UPDATE(P, Pp, x, v, xp, vp, z, a.r)
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) x[c] = xp[c], v[c] = vp[c];
                    P[0] = Pp[0];
                    P[1] = Pp[1];
                }
            }
            if (row < C) {
                const size_t at = (size_t)row * R + r;
                a.sm_id[at] = id;
                a.sm_state[at] = (signed char)(seen ? TRAJ_OBSERVED : TRAJ_FILLED);
                a.sm_src_frame[at] = src_f;
                a.sm_src_slot[at] = src_j;
                atomicMax(&a.sm_count[r], row + 1);                 // an integer maximum: the order does not matter
                n_obs += seen ? 1 : 0;
                n_fill += seen ? 0 : 1;
                if (f < last) {                                    // what the backward pass reads
                    double *w = a.ws + (size_t)r * C + row;
                    const size_t plane = (size_t)R * C;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        w[(WS_X + c) * plane] = x[c];
                        w[(WS_V + c) * plane] = v[c];
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        w[(WS_P + 6 * c) * plane] = P[c].xx;
                        w[(WS_P + 6 * c + 1) * plane] = P[c].xv;
                        w[(WS_P + 6 * c + 2) * plane] = P[c].vv;
                    }
                }
                if (f > first) {
                    double *w = a.ws + (size_t)r * C + row;
                    const size_t plane = (size_t)R * C;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        w[(WS_XP + c) * plane] = xp[c];
                        w[(WS_VP + c) * plane] = vp[c];
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        w[(WS_PP + 6 * c) * plane] = Pp[c].xx;
                        w[(WS_PP + 6 * c + 1) * plane] = Pp[c].xv;
                        w[(WS_PP + 6 * c + 2) * plane] = Pp[c].vv;
                    }
                }
            }
        }
        if (n_obs) atomicAdd(&counts_s[0], n_obs);                  // integer adds in LDS: the order does not matter
        if (n_fill) atomicAdd(&counts_s[1], n_fill);

        // ---- the forecast: the filtered state at `last`, shifts extrapolated, scales held ----------------------------------------------------
        if (forecast) {
            int row = 0;
            for (int k = 0; k < m; ++k) row += olast_s[k][tid] >= live_from ? 1 : 0;
            if (row < C) {
                const float2 vel = make_float2((float)(((double)a.W * v[1]) * 0.5), (float)(((double)a.H * v[3]) * 0.5));
                for (int k = 1; k <= Hz; ++k) {
                    const double mm = (double)(F - 1 - last + k);
                    const float4 w4 = make_float4((float)x[0], (float)(x[1] + mm * v[1]), (float)x[2], (float)(x[3] + mm * v[3]));
                    const size_t col = (size_t)s * Hz + (k - 1), at = (size_t)row * N + col;
                    reinterpret_cast<float4 *>(a.fc_where)[at] = w4;
                    reinterpret_cast<float4 *>(a.fc_boxes)[at] = attention_box4(w4, Wf, Hf);
                    reinterpret_cast<float2 *>(a.fc_velocity)[at] = vel;
                    a.fc_id[at] = id;
                    a.fc_state[at] = (signed char)TRAJ_FORECAST;
                    a.fc_src_frame[at] = src_f;
                    a.fc_src_slot[at] = src_j;
                    atomicMax(&a.fc_count[col], row + 1);
                }
            }
        }

        // ---- backward: xs[last] = x, vs[last] = v, then last - 1 down to first ----------------------------------------------------------------
        double xs[4], vs[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) xs[c] = x[c], vs[c] = v[c];
        int row_next = -1;                                          // the row in frame f + 1
        for (int f = last; f >= first; --f) {
            const int r = s * F + f;
            int row = 0;
            for (int k = 0; k < m; ++k) row += olast_s[k][tid] >= f ? 1 : 0;
            if (f < last && row < C && row_next < C) {
                const size_t plane = (size_t)R * C;
                const double *w = a.ws + (size_t)r * C + row, *wn = a.ws + (size_t)(r + 1) * C + row_next;
                TRAJ_BACK(w, wn, plane, xs, vs)
            }
            if (row < C) {
                const size_t at = (size_t)row * R + r;
                const float4 w4 = make_float4((float)xs[0], (float)xs[1], (float)xs[2], (float)xs[3]);
                reinterpret_cast<float4 *>(a.sm_where)[at] = w4;
                reinterpret_cast<float4 *>(a.sm_boxes)[at] = attention_box4(w4, Wf, Hf);
                reinterpret_cast<float2 *>(a.sm_velocity)[at] =
                    make_float2((float)(((double)a.W * vs[1]) * 0.5), (float)(((double)a.H * vs[3]) * 0.5));
            }
            row_next = row;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int *c = a.sm_counts + (size_t)s * 3;
        c[TRAJ_OBSERVED] = counts_s[0];
        c[TRAJ_FILLED] = counts_s[1];
        c[TRAJ_ABSENT] = C * F - counts_s[0] - counts_s[1];
    }
}

extern "C" size_t air_track_smooth_workspace_bytes(int C, int R) {
    if (C < 1 || C > TRAJ_MAXT || R < 1) return 0;
    return (size_t)TRAJ_WS_DOUBLES * sizeof(double) * (size_t)C * (size_t)R;
}

extern "C" int air_track_smooth(const float *where, const int *num_objects, const int *track_id, const int *num_tracks,
                                const int *track_first, const int *track_last, int T, int S, int F, int R, int C, int Hz, int max_age,
                                int H, int W, double q_shift, double q_scale, double r, double velocity_var, double *ws,
                                size_t ws_bytes, float *sm_where, float *sm_boxes, int *sm_id, signed char *sm_state,
                                int *sm_src_frame, int *sm_src_slot, float *sm_velocity, int *sm_count, int *sm_counts,
                                float *fc_where, float *fc_boxes, int *fc_id, signed char *fc_state, int *fc_src_frame,
                                int *fc_src_slot, float *fc_velocity, int *fc_count, void *stream) {
    AIR_REQUIRE(where && num_objects && track_id && num_tracks && track_first && track_last && ws && sm_where && sm_boxes && sm_id &&
                sm_state && sm_src_frame && sm_src_slot && sm_velocity && sm_count && sm_counts, AIR_E_NULL);
    AIR_REQUIRE(Hz >= 0 && Hz <= TRAJ_MAX_HORIZON, AIR_E_SHAPE);
    AIR_REQUIRE(Hz == 0 || (fc_where && fc_boxes && fc_id && fc_state && fc_src_frame && fc_src_slot && fc_velocity && fc_count),
                AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRAJ_MAXT && S > 0 && F > 0 && H > 0 && W > 0 && max_age >= 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= TRAJ_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    const long want_c = (long)T * ((long)max_age + 1) < TRAJ_MAXT ? (long)T * ((long)max_age + 1) : TRAJ_MAXT;
    AIR_REQUIRE((long)C == want_c && (long)C * R <= (long)INT_MAX / 4, AIR_E_SHAPE);
    AIR_REQUIRE(traj_noise_check(q_shift, q_scale, r, velocity_var) == AIR_OK, AIR_E_SHAPE);
    AIR_REQUIRE(ws_bytes >= air_track_smooth_workspace_bytes(C, R), AIR_E_WORKSPACE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(sm_where) && air_aligned16(sm_boxes) &&
                (Hz == 0 || (air_aligned16(fc_where) && air_aligned16(fc_boxes))), AIR_E_ALIGN);
    AIR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sm_velocity) & 7u) == 0 &&
                (reinterpret_cast<uintptr_t>(fc_velocity) & 7u) == 0, AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(num_tracks) | reinterpret_cast<uintptr_t>(track_first) |
                           reinterpret_cast<uintptr_t>(track_last) | reinterpret_cast<uintptr_t>(sm_id) |
                           reinterpret_cast<uintptr_t>(sm_src_frame) | reinterpret_cast<uintptr_t>(sm_src_slot) |
                           reinterpret_cast<uintptr_t>(sm_count) | reinterpret_cast<uintptr_t>(sm_counts) |
                           reinterpret_cast<uintptr_t>(fc_id) | reinterpret_cast<uintptr_t>(fc_src_frame) |
                           reinterpret_cast<uintptr_t>(fc_src_slot) | reinterpret_cast<uintptr_t>(fc_count);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    TrajSmoothArgs a;
    a.where = where, a.num_objects = num_objects, a.track_id = track_id, a.num_tracks = num_tracks;
    a.track_first = track_first, a.track_last = track_last, a.ws = ws;
    a.sm_where = sm_where, a.sm_boxes = sm_boxes, a.sm_velocity = sm_velocity;
    a.fc_where = fc_where, a.fc_boxes = fc_boxes, a.fc_velocity = fc_velocity;
    a.sm_id = sm_id, a.sm_src_frame = sm_src_frame, a.sm_src_slot = sm_src_slot, a.sm_count = sm_count, a.sm_counts = sm_counts;
    a.fc_id = fc_id, a.fc_src_frame = fc_src_frame, a.fc_src_slot = fc_src_slot, a.fc_count = fc_count;
    a.sm_state = sm_state, a.fc_state = fc_state;
    a.q[0] = q_shift, a.q[1] = q_scale, a.r = r, a.velocity_var = velocity_var;
    a.T = T, a.S = S, a.F = F, a.C = C, a.Hz = Hz, a.max_age = max_age, a.H = H, a.W = W;
    hipLaunchKernelGGL(track_smooth_kernel, dim3((unsigned)S), dim3(TRAJ_SMOOTH_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// fill
// ============================================================================================================
struct TrajFillArgs {
    const float *what, *glimpse, *score;
    const signed char *state;
    const int *src_frame, *src_slot;
    float *out_what, *out_glimpse, *out_score;
    int T, F, R, C, N, per_seq, A, G, what_vec, glimpse_vec;
};

// One wavefront per (row c, column n) of the table; column n belongs to sequence n / per_seq (per_seq = F for the completed table,
// the horizon for the forecast table).  A row that is ABSENT, or whose source is outside the provider's rows, gets zeros.
__global__ __launch_bounds__(TRAJ_THREADS) void track_fill_kernel(TrajFillArgs a) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * (TRAJ_THREADS / 64) + wid;
    if (e >= (long)a.C * a.N) return;
    const int n = (int)(e % a.N);
    const int s = n / a.per_seq;
    const int st = (int)a.state[e], sf = a.src_frame[e], sj = a.src_slot[e];
    const bool has = st != TRAJ_ABSENT && sf >= 0 && sf < a.F && sj >= 0 && sj < a.T;
    const size_t from = has ? (size_t)sj * a.R + (size_t)s * a.F + sf : 0;
    copy_row_bits_or_zero(has ? a.what + from * a.A : nullptr, a.out_what + (size_t)e * a.A, a.A, a.what_vec != 0, lane);
    copy_row_bits_or_zero(has ? a.glimpse + from * a.G : nullptr, a.out_glimpse + (size_t)e * a.G, a.G, a.glimpse_vec != 0, lane);
    if (lane == 0) reinterpret_cast<unsigned *>(a.out_score)[e] = has ? reinterpret_cast<const unsigned *>(a.score)[from] : 0u;
}

extern "C" int air_track_fill(const float *what, const float *glimpse, const float *score, const signed char *state,
                              const int *src_frame, const int *src_slot, int T, int F, int R, int C, int N, int per_seq, int A, int G,
                              float *out_what, float *out_glimpse, float *out_score, void *stream) {
    AIR_REQUIRE(what && glimpse && score && state && src_frame && src_slot && out_what && out_glimpse && out_score, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRAJ_MAXT && C >= 1 && C <= TRAJ_MAXT && F > 0 && R > 0 && N > 0 && per_seq > 0 && A > 0 && G > 0,
                AIR_E_SHAPE);
    AIR_REQUIRE(R % F == 0 && N % per_seq == 0 && N / per_seq == R / F, AIR_E_SHAPE);
    AIR_REQUIRE((long)C * N <= (long)INT_MAX && (long)T * R <= (long)INT_MAX, AIR_E_SHAPE);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(score) |
                           reinterpret_cast<uintptr_t>(src_frame) | reinterpret_cast<uintptr_t>(src_slot) |
                           reinterpret_cast<uintptr_t>(out_what) | reinterpret_cast<uintptr_t>(out_glimpse) |
                           reinterpret_cast<uintptr_t>(out_score);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    TrajFillArgs a = {what, glimpse, score, state, src_frame, src_slot, out_what, out_glimpse, out_score, T, F, R, C, N, per_seq, A, G,
                      A % 4 == 0 && air_aligned16(what) && air_aligned16(out_what),
                      G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(out_glimpse)};
    const long waves = (long)C * N;
    hipLaunchKernelGGL(track_fill_kernel, dim3((unsigned)air_cdiv(waves, TRAJ_THREADS / 64)), dim3(TRAJ_THREADS), 0,
                       air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// streams: fixed-lag smoothing and forecasts per chunk (include/air_hip.h states the rule and the layout of the carried state)
// ============================================================================================================
#define TRAJ_MAX_LAG 16
#define TRAJ_RING_INTS 4                 // per (frame, table row): id, state, the last sighting at or before the frame (frame, slot)
#define TRAJ_PLANE TRAJ_MAXT             // table row fastest: plane p of frame d is ring[((s D + d) 28 + p) 32 + row]
enum { SM_LIVE = 0, SM_ID, SM_AGE, SM_FIRST, SM_LAST_FRAME, SM_LAST_SLOT, SM_FIELDS };
enum { RING_ID = 0, RING_STATE, RING_SRC_FRAME, RING_SRC_SLOT };

struct TrajTable {
    float *where, *boxes, *velocity;
    int *id, *src_frame, *src_slot, *count;
    signed char *state;
};

struct TrajStreamArgs {
    const float *where;
    const int *num_objects, *track_id, *valid;
    int *seq, *slots, *ring_i;
    double *ring;
    TrajTable sm, fc;                    // (the tail launch: sm is the tail table, emit_frame the tail's frames)
    int *emit_frame, *num_emitted, *sm_counts;
    double q[2], r, velocity_var;
    int T, S, F, C, L, Hz, D, max_age, H, W;
};

// the sections of the packed state: seq [S,2], slots [S,6,32], ring_i [S,D,4,32] (int32), ring [S,D,28,32] (float64)
static inline size_t traj_stream_state_ints(int S, int D) {
    return (size_t)S * (2 + SM_FIELDS * TRAJ_MAXT + (size_t)D * TRAJ_RING_INTS * TRAJ_MAXT);
}

extern "C" size_t air_track_smooth_stream_state_bytes(int S, int D) {
    if (S < 1 || D < 1 || (long)S * D > (long)INT_MAX / (TRAJ_WS_DOUBLES * TRAJ_MAXT)) return 0;
    return traj_stream_state_ints(S, D) * sizeof(int) + (size_t)S * D * TRAJ_WS_DOUBLES * TRAJ_MAXT * sizeof(double);
}

static inline void traj_stream_state(TrajStreamArgs &a, void *state) {
    a.seq = reinterpret_cast<int *>(state);
    a.slots = a.seq + (size_t)a.S * 2;
    a.ring_i = a.slots + (size_t)a.S * SM_FIELDS * TRAJ_MAXT;
    a.ring = reinterpret_cast<double *>(a.seq + traj_stream_state_ints(a.S, a.D));      // (an even number of ints: 8-byte aligned)
}

// the `per_seq` columns of sequence s of a table of N columns start ABSENT
__device__ __forceinline__ void traj_table_absent(const TrajTable &t, size_t N, int s, int per_seq, int C, int tid) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = tid; e < C * per_seq; e += TRAJ_SMOOTH_THREADS) {
        const int c = e / per_seq, f = e - c * per_seq;
        const size_t at = (size_t)c * N + (size_t)s * per_seq + f;
        reinterpret_cast<float4 *>(t.where)[at] = z4;
        reinterpret_cast<float4 *>(t.boxes)[at] = z4;
        t.velocity[2 * at] = 0.f;
        t.velocity[2 * at + 1] = 0.f;
        t.id[at] = -1;
        t.state[at] = (signed char)TRAJ_ABSENT;
        t.src_frame[at] = -1;
        t.src_slot[at] = -1;
    }
    for (int f = tid; f < per_seq; f += TRAJ_SMOOTH_THREADS) t.count[(size_t)s * per_seq + f] = 0;
}

// Frame g of sequence s smoothed with the frames up to hi (g <= hi < g + D) into column `col` of table t; every lane of the wavefront
// calls it, lane k < 32 is table row k.  The rows: the tracks live in g that are sighted in g .. hi, in ascending id (a count of
// integers over the lanes); each lane runs the backward pass of its own track from the last sighting within g .. hi down to g, over
// the ring entries it wrote itself.  n_obs / n_fill: the rows written per state, the same in every lane.
__device__ __forceinline__ void traj_emit_column(const TrajStreamArgs &a, const TrajTable &t, size_t N, size_t col, int s, int g, int hi,
                                                 int lane, int &n_obs, int &n_fill) {
#pragma clang fp contract(off)
    const int D = a.D, k = lane & (TRAJ_MAXT - 1);
    const size_t seq_d = (size_t)s * D;
    int rid = -1, st = TRAJ_ABSENT, sf = -1, sj = -1, la = -1;
    if (lane < TRAJ_MAXT) {
        const int *ri = a.ring_i + (seq_d + g % D) * (TRAJ_RING_INTS * TRAJ_MAXT) + k;
        rid = ri[RING_ID * TRAJ_MAXT], st = ri[RING_STATE * TRAJ_MAXT];
        sf = ri[RING_SRC_FRAME * TRAJ_MAXT], sj = ri[RING_SRC_SLOT * TRAJ_MAXT];
    }
    if (rid >= 0)
        for (int f = g; f <= hi; ++f) {
            const int *e = a.ring_i + (seq_d + f % D) * (TRAJ_RING_INTS * TRAJ_MAXT) + k;
            if (e[RING_ID * TRAJ_MAXT] != rid) break;              // retired, the row free or another track's from here on
            if (e[RING_STATE * TRAJ_MAXT] == TRAJ_OBSERVED) la = f;
        }
    const bool spans = la >= 0;
    const int key = spans ? rid : INT_MAX;
    int row = 0;
    for (int kk = 0; kk < TRAJ_MAXT; ++kk) row += __shfl(key, kk) < rid ? 1 : 0;      // (an id lives in one table row)
    const bool writes = spans && row < a.C;
    if (writes) {
        const int plane = TRAJ_PLANE;
        const double *wl = a.ring + (seq_d + la % D) * (TRAJ_WS_DOUBLES * TRAJ_PLANE) + k;
        double xs[4], vs[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) xs[c] = wl[(WS_X + c) * plane], vs[c] = wl[(WS_V + c) * plane];
        for (int f = la - 1; f >= g; --f) {
            const double *w = a.ring + (seq_d + f % D) * (TRAJ_WS_DOUBLES * TRAJ_PLANE) + k;
            const double *wn = a.ring + (seq_d + (f + 1) % D) * (TRAJ_WS_DOUBLES * TRAJ_PLANE) + k;
            TRAJ_BACK(w, wn, plane, xs, vs)
        }
        const size_t at = (size_t)row * N + col;
        const float4 w4 = make_float4((float)xs[0], (float)xs[1], (float)xs[2], (float)xs[3]);
        reinterpret_cast<float4 *>(t.where)[at] = w4;
        reinterpret_cast<float4 *>(t.boxes)[at] = attention_box4(w4, (float)a.W, (float)a.H);
        reinterpret_cast<float2 *>(t.velocity)[at] =
            make_float2((float)(((double)a.W * vs[1]) * 0.5), (float)(((double)a.H * vs[3]) * 0.5));
        t.id[at] = rid;
        t.state[at] = (signed char)st;
        t.src_frame[at] = sf;
        t.src_slot[at] = sj;
    }
    const int n_rows = __popcll(__ballot(writes));
    n_obs += __popcll(__ballot(writes && st == TRAJ_OBSERVED));
    n_fill += __popcll(__ballot(writes && st == TRAJ_FILLED));
    if (lane == 0) t.count[col] = n_rows;
}

// One workgroup of one wavefront per sequence, lane k < 32 = row k of the smoother's own track table.  The chunk's valid frames are
// walked in order with the table and the filter state in registers: sightings by id (the lowest slot that carries it), births into
// the lowest free row in ascending slot, ageing and retirement as the tracker does them; every frame's filtered and predicted
// values go to the ring.  Then the frames that became final, then the forecast of the live tracks.
__global__ __launch_bounds__(TRAJ_SMOOTH_THREADS) void track_smooth_stream_kernel(TrajStreamArgs a) {
#pragma clang fp contract(off)
    const int T = a.T, F = a.F, C = a.C, L = a.L, Hz = a.Hz, D = a.D, R = a.S * F;
    const int s = blockIdx.x, lane = threadIdx.x, k = lane & (TRAJ_MAXT - 1);
    const bool row_lane = lane < TRAJ_MAXT;
    const size_t N = (size_t)a.S * Hz, seq_d = (size_t)s * D;
    const int plane = TRAJ_PLANE;
    const double q2[2] = {0.5 * a.q[0], 0.5 * a.q[1]}, q4[2] = {0.25 * a.q[0], 0.25 * a.q[1]};
    const int a0 = a.seq[2 * s] > 0 ? a.seq[2 * s] : 0, next_emit = a.seq[2 * s + 1];
    int nv = a.valid[s];
    nv = nv < 0 ? 0 : (nv > F ? F : nv);
    const int b = a0 + nv;
    traj_table_absent(a.sm, (size_t)R, s, F, C, lane);
    if (Hz > 0) traj_table_absent(a.fc, N, s, Hz, C, lane);
    for (int e = lane; e < F; e += TRAJ_SMOOTH_THREADS) a.emit_frame[(size_t)s * F + e] = -1;

    // ---- the table and the filter state of the live rows (the ring entry of frame a0 - 1) ------------------------------------------------
    int *sl = a.slots + (size_t)s * SM_FIELDS * TRAJ_MAXT + k;
    int live = 0, id = -1, age = 0, first = -1, lf = -1, lj = -1;
    if (row_lane) {
        live = sl[SM_LIVE * TRAJ_MAXT], id = sl[SM_ID * TRAJ_MAXT], age = sl[SM_AGE * TRAJ_MAXT];
        first = sl[SM_FIRST * TRAJ_MAXT], lf = sl[SM_LAST_FRAME * TRAJ_MAXT], lj = sl[SM_LAST_SLOT * TRAJ_MAXT];
    }
    double x[4] = {0.0, 0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
    TrajCov P[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (live && a0 > 0 && nv > 0) {
        const double *w = a.ring + (seq_d + (a0 - 1) % D) * (TRAJ_WS_DOUBLES * TRAJ_PLANE) + k;
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = w[(WS_X + c) * plane], v[c] = w[(WS_V + c) * plane];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            P[c].xx = w[(WS_P + 6 * c) * plane];
            P[c].xv = w[(WS_P + 6 * c + 1) * plane];
            P[c].vv = w[(WS_P + 6 * c + 2) * plane];
        }
    }

    // ---- forward: the chunk's valid frames ---------------------------------------------------------------------------------------------
    for (int f = 0; f < nv; ++f) {
        const int g = a0 + f, r = s * F + f;
        int n = a.num_objects[r];
        n = n < 0 ? 0 : (n > T ? T : n);
        const int my_id = lane < n ? a.track_id[(size_t)lane * R + r] : -1;      // (n <= 32: slot j in lane j)
        int seen_j = -1;
        bool born = false;
        for (int j = 0; j < n; ++j) {                              // the same in every lane
            const int idj = __shfl(my_id, j);
            if (idj < 0) continue;
            const bool mine = live && id == idj;
            if (__ballot(mine)) {
                if (mine && seen_j < 0) seen_j = j;                // the lowest slot that carries the id
            } else {
                const unsigned long long free_rows = __ballot(row_lane && !live);
                if (free_rows && lane == __ffsll((long long)free_rows) - 1) {      // a birth into the lowest free row
                    live = 1, id = idj, age = 0, first = g, seen_j = j;
                    born = true;
                }
            }
        }
        int *ri = a.ring_i + (seq_d + g % D) * (TRAJ_RING_INTS * TRAJ_MAXT) + k;
        if (live) {
            const bool seen = seen_j >= 0;
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (seen) {
                const float4 w4 = reinterpret_cast<const float4 *>(a.where)[(size_t)seen_j * R + r];
                z[0] = (double)w4.x, z[1] = (double)w4.y, z[2] = (double)w4.z, z[3] = (double)w4.w;
            }
            TrajCov Pp[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
            double xp[4] = {0.0, 0.0, 0.0, 0.0}, vp[4] = {0.0, 0.0, 0.0, 0.0};
            if (born) {                                            // start: x = z, v = 0, P = (r, 0, velocity_var)
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c] = z[c], v[c] = 0.0;
                P[0].xx = P[1].xx = a.r;
                P[0].xv = P[1].xv = 0.0;
                P[0].vv = P[1].vv = a.velocity_var;
            } else {
#pragma unroll
                for (int c = 0; c < 2; ++c) Pp[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) xp[c] = x[c] + v[c], vp[c] = v[c];
                if (seen) {
                    TRAJ_UPDATE(P, Pp, x, v, xp, vp, z, a.r)
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) x[c] = xp[c], v[c] = vp[c];
                    P[0] = Pp[0];
                    P[1] = Pp[1];
                }
            }
            if (seen) age = 0, lf = g, lj = seen_j;
            else ++age;
            double *w = a.ring + (seq_d + g % D) * (TRAJ_WS_DOUBLES * TRAJ_PLANE) + k;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                w[(WS_X + c) * plane] = x[c];
                w[(WS_V + c) * plane] = v[c];
                w[(WS_XP + c) * plane] = xp[c];
                w[(WS_VP + c) * plane] = vp[c];
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                w[(WS_P + 6 * c) * plane] = P[c].xx;
                w[(WS_P + 6 * c + 1) * plane] = P[c].xv;
                w[(WS_P + 6 * c + 2) * plane] = P[c].vv;
                w[(WS_PP + 6 * c) * plane] = Pp[c].xx;
                w[(WS_PP + 6 * c + 1) * plane] = Pp[c].xv;
                w[(WS_PP + 6 * c + 2) * plane] = Pp[c].vv;
            }
            ri[RING_ID * TRAJ_MAXT] = id;
            ri[RING_STATE * TRAJ_MAXT] = seen ? TRAJ_OBSERVED : TRAJ_FILLED;
            ri[RING_SRC_FRAME * TRAJ_MAXT] = lf;
            ri[RING_SRC_SLOT * TRAJ_MAXT] = lj;
            if (age > a.max_age) live = 0, id = -1, age = 0, first = -1, lf = -1, lj = -1;      // retired: the tracker's ageing
        } else if (row_lane) {
            ri[RING_ID * TRAJ_MAXT] = -1;
            ri[RING_STATE * TRAJ_MAXT] = TRAJ_ABSENT;
            ri[RING_SRC_FRAME * TRAJ_MAXT] = -1;
            ri[RING_SRC_SLOT * TRAJ_MAXT] = -1;
        }
    }
    if (row_lane) {
        sl[SM_LIVE * TRAJ_MAXT] = live, sl[SM_ID * TRAJ_MAXT] = id, sl[SM_AGE * TRAJ_MAXT] = age;
        sl[SM_FIRST * TRAJ_MAXT] = first, sl[SM_LAST_FRAME * TRAJ_MAXT] = lf, sl[SM_LAST_SLOT * TRAJ_MAXT] = lj;
    }
    __syncthreads();                                               // the ABSENT fill is behind; the rows overwrite it

    // ---- the frames that became final: g + L < b ---------------------------------------------------------------------------------------
    const int emit_end = b - L > 0 ? b - L : 0;
    int n_obs = 0, n_fill = 0, e = 0;
    for (int g = next_emit > 0 ? next_emit : 0; g < emit_end && e < F; ++g, ++e) {
        traj_emit_column(a, a.sm, (size_t)R, (size_t)s * F + e, s, g, g + L, lane, n_obs, n_fill);
        if (lane == 0) a.emit_frame[(size_t)s * F + e] = g;
    }
    if (lane == 0) {
        a.num_emitted[s] = e;
        int *c = a.sm_counts + (size_t)s * 3;
        c[TRAJ_OBSERVED] = n_obs;
        c[TRAJ_FILLED] = n_fill;
        c[TRAJ_ABSENT] = C * e - n_obs - n_fill;
        a.seq[2 * s] = b;
        a.seq[2 * s + 1] = emit_end;
    }

    // ---- the forecast: the filtered state at the last sighting, shifts extrapolated, scales held ---------------------------------------------
    if (Hz > 0 && b > 0) {
        const int key = live ? id : INT_MAX;
        int row = 0;
        for (int kk = 0; kk < TRAJ_MAXT; ++kk) row += __shfl(key, kk) < id ? 1 : 0;
        const bool writes = live && lf >= 0 && row < C;            // (a live row has a sighting: lf >= 0 in every state this kernel writes)
        if (writes) {
            const double *w = a.ring + (seq_d + lf % D) * (TRAJ_WS_DOUBLES * TRAJ_PLANE) + k;
            double xl[4], vl[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) xl[c] = w[(WS_X + c) * plane], vl[c] = w[(WS_V + c) * plane];
            const float2 vel = make_float2((float)(((double)a.W * vl[1]) * 0.5), (float)(((double)a.H * vl[3]) * 0.5));
            for (int kf = 1; kf <= Hz; ++kf) {
                const double mm = (double)(b - 1 - lf + kf);
                const float4 w4 = make_float4((float)xl[0], (float)(xl[1] + mm * vl[1]), (float)xl[2], (float)(xl[3] + mm * vl[3]));
                const size_t at = (size_t)row * N + (size_t)s * Hz + (kf - 1);
                reinterpret_cast<float4 *>(a.fc.where)[at] = w4;
                reinterpret_cast<float4 *>(a.fc.boxes)[at] = attention_box4(w4, (float)a.W, (float)a.H);
                reinterpret_cast<float2 *>(a.fc.velocity)[at] = vel;
                a.fc.id[at] = id;
                a.fc.state[at] = (signed char)TRAJ_FORECAST;
                a.fc.src_frame[at] = lf;
                a.fc.src_slot[at] = lj;
            }
        }
        const int n_rows = __popcll(__ballot(writes));
        for (int kf = lane; kf < Hz; kf += TRAJ_SMOOTH_THREADS) a.fc.count[(size_t)s * Hz + kf] = n_rows;
    }
}

// the frames max(0, b - L) .. b - 1, not final yet, smoothed with what is known; the state is only read
__global__ __launch_bounds__(TRAJ_SMOOTH_THREADS) void track_smooth_tail_kernel(TrajStreamArgs a) {
    const int L = a.L, s = blockIdx.x, lane = threadIdx.x;
    const size_t N = (size_t)a.S * L;
    const int b = a.seq[2 * s], g0 = b - L > 0 ? b - L : 0;
    traj_table_absent(a.sm, N, s, L, a.C, lane);
    for (int j = lane; j < L; j += TRAJ_SMOOTH_THREADS) a.emit_frame[(size_t)s * L + j] = g0 + j < b ? g0 + j : -1;
    __syncthreads();
    int n_obs = 0, n_fill = 0;
    for (int j = 0; j < L && g0 + j < b; ++j) traj_emit_column(a, a.sm, N, (size_t)s * L + j, s, g0 + j, b - 1, lane, n_obs, n_fill);
}

static int traj_table_check(const TrajTable &t) {
    AIR_REQUIRE(t.where && t.boxes && t.id && t.state && t.src_frame && t.src_slot && t.velocity && t.count, AIR_E_NULL);
    AIR_REQUIRE(air_aligned16(t.where) && air_aligned16(t.boxes) && (reinterpret_cast<uintptr_t>(t.velocity) & 7u) == 0, AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(t.id) | reinterpret_cast<uintptr_t>(t.src_frame) |
                           reinterpret_cast<uintptr_t>(t.src_slot) | reinterpret_cast<uintptr_t>(t.count);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    return AIR_OK;
}

// the checks the stream entries share: the shapes, the rule's arguments, the state
static int traj_stream_check(int T, int S, int C, int L, int D, int max_age, int H, int W, const void *state, size_t state_bytes) {
    AIR_REQUIRE(state, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRAJ_MAXT && S > 0 && H > 0 && W > 0 && max_age >= 0, AIR_E_SHAPE);
    AIR_REQUIRE(L >= max_age && L <= TRAJ_MAX_LAG && D >= 1, AIR_E_SHAPE);
    const long want_c = (long)T * ((long)max_age + 1) < TRAJ_MAXT ? (long)T * ((long)max_age + 1) : TRAJ_MAXT;
    AIR_REQUIRE((long)C == want_c, AIR_E_SHAPE);
    const size_t need = air_track_smooth_stream_state_bytes(S, D);
    AIR_REQUIRE(need > 0, AIR_E_SHAPE);
    AIR_REQUIRE(state_bytes >= need, AIR_E_WORKSPACE);
    AIR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0, AIR_E_ALIGN);
    return AIR_OK;
}

extern "C" int air_track_smooth_stream(const float *where, const int *num_objects, const int *track_id, const int *valid, int T, int S,
                                       int F, int R, int C, int L, int Hz, int D, int max_age, int H, int W, double q_shift,
                                       double q_scale, double r, double velocity_var, void *state, size_t state_bytes, float *sm_where,
                                       float *sm_boxes, int *sm_id, signed char *sm_state, int *sm_src_frame, int *sm_src_slot,
                                       float *sm_velocity, int *sm_count, int *sm_counts, int *emit_frame, int *num_emitted,
                                       float *fc_where, float *fc_boxes, int *fc_id, signed char *fc_state, int *fc_src_frame,
                                       int *fc_src_slot, float *fc_velocity, int *fc_count, void *stream) {
    TrajStreamArgs a;
    a.sm = {sm_where, sm_boxes, sm_velocity, sm_id, sm_src_frame, sm_src_slot, sm_count, sm_state};
    a.fc = {fc_where, fc_boxes, fc_velocity, fc_id, fc_src_frame, fc_src_slot, fc_count, fc_state};
    AIR_REQUIRE(where && num_objects && track_id && valid && sm_counts && emit_frame && num_emitted, AIR_E_NULL);
    int st = traj_table_check(a.sm);
    AIR_REQUIRE(st == AIR_OK, st);
    AIR_REQUIRE(Hz >= 0 && Hz <= TRAJ_MAX_HORIZON, AIR_E_SHAPE);
    if (Hz > 0) {
        st = traj_table_check(a.fc);
        AIR_REQUIRE(st == AIR_OK, st);
    }
    AIR_REQUIRE(F > 0 && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    st = traj_stream_check(T, S, C, L, D, max_age, H, W, state, state_bytes);
    AIR_REQUIRE(st == AIR_OK, st);
    AIR_REQUIRE((long)F * T <= TRAJ_MAX_IDS && (long)C * R <= (long)INT_MAX / 4, AIR_E_SHAPE);
    AIR_REQUIRE((long)D >= (long)F + L + max_age, AIR_E_SHAPE);    // the ring: frame a - L - max_age is read, a + F - 1 written
    AIR_REQUIRE(traj_noise_check(q_shift, q_scale, r, velocity_var) == AIR_OK, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(valid) | reinterpret_cast<uintptr_t>(sm_counts) |
                           reinterpret_cast<uintptr_t>(emit_frame) | reinterpret_cast<uintptr_t>(num_emitted);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    a.where = where, a.num_objects = num_objects, a.track_id = track_id, a.valid = valid;
    a.emit_frame = emit_frame, a.num_emitted = num_emitted, a.sm_counts = sm_counts;
    a.q[0] = q_shift, a.q[1] = q_scale, a.r = r, a.velocity_var = velocity_var;
    a.T = T, a.S = S, a.F = F, a.C = C, a.L = L, a.Hz = Hz, a.D = D, a.max_age = max_age, a.H = H, a.W = W;
    traj_stream_state(a, state);
    hipLaunchKernelGGL(track_smooth_stream_kernel, dim3((unsigned)S), dim3(TRAJ_SMOOTH_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_track_smooth_tail(int T, int S, int C, int L, int D, int max_age, int H, int W, const void *state, size_t state_bytes,
                                     float *tl_where, float *tl_boxes, int *tl_id, signed char *tl_state, int *tl_src_frame,
                                     int *tl_src_slot, float *tl_velocity, int *tl_count, int *tail_frame, void *stream) {
    int st = traj_stream_check(T, S, C, L, D, max_age, H, W, state, state_bytes);
    AIR_REQUIRE(st == AIR_OK, st);
    AIR_REQUIRE((long)D >= (long)L + max_age && (long)C * S * (L > 0 ? L : 1) <= (long)INT_MAX / 4, AIR_E_SHAPE);
    if (L == 0) return AIR_OK;                                     // (max_age = 0 and no lag: every frame is final when it is seen)
    TrajStreamArgs a;
    a.sm = {tl_where, tl_boxes, tl_velocity, tl_id, tl_src_frame, tl_src_slot, tl_count, tl_state};
    a.fc = a.sm;
    st = traj_table_check(a.sm);
    AIR_REQUIRE(st == AIR_OK, st);
    AIR_REQUIRE(tail_frame, AIR_E_NULL);
    AIR_REQUIRE((reinterpret_cast<uintptr_t>(tail_frame) & 3u) == 0, AIR_E_ALIGN);
    a.where = nullptr, a.num_objects = a.track_id = a.valid = nullptr;
    a.emit_frame = tail_frame, a.num_emitted = nullptr, a.sm_counts = nullptr;
    a.q[0] = a.q[1] = a.r = a.velocity_var = 0.0;
    a.T = T, a.S = S, a.F = 0, a.C = C, a.L = L, a.Hz = 0, a.D = D, a.max_age = max_age, a.H = H, a.W = W;
    traj_stream_state(a, const_cast<void *>(state));
    hipLaunchKernelGGL(track_smooth_tail_kernel, dim3((unsigned)S), dim3(TRAJ_SMOOTH_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ---- the ring of provider rows: the stash of a chunk's valid rows, and the fill of a table's rows from it --------------------------------
struct TrajStashArgs {
    const float *what, *glimpse, *score;
    const int *valid, *seq;
    float *ring_what, *ring_glimpse, *ring_score;
    int T, S, F, R, A, G, D, what_vec, glimpse_vec;
};

// One wavefront per (slot j, chunk row r): row (j, s F + f) with f < clip(valid[s], 0, F) goes to the ring at frame
// (frames_seen[s] + f) mod D; runs BEFORE air_track_smooth_stream moves frames_seen.
__global__ __launch_bounds__(TRAJ_THREADS) void track_stash_kernel(TrajStashArgs a) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * (TRAJ_THREADS / 64) + wid;
    if (e >= (long)a.T * a.R) return;
    const int r = (int)(e % a.R), j = (int)(e / a.R);
    const int s = r / a.F, f = r - s * a.F;
    int nv = a.valid[s];
    nv = nv < 0 ? 0 : (nv > a.F ? a.F : nv);
    const int seen = a.seq[2 * s];
    if (f >= nv || seen < 0) return;                               // (frames_seen is never negative in a state the kernels wrote)
    const int d = (seen + f) % a.D;
    const size_t to = ((size_t)s * a.D + d) * a.T + j;
    copy_row_bits_or_zero(a.what + (size_t)e * a.A, a.ring_what + to * a.A, a.A, a.what_vec != 0, lane);
    copy_row_bits_or_zero(a.glimpse + (size_t)e * a.G, a.ring_glimpse + to * a.G, a.G, a.glimpse_vec != 0, lane);
    if (lane == 0) reinterpret_cast<unsigned *>(a.ring_score)[to] = reinterpret_cast<const unsigned *>(a.score)[e];
}

extern "C" int air_track_stash(const float *what, const float *glimpse, const float *score, const int *valid, const void *state, int T,
                               int S, int F, int R, int A, int G, int D, float *ring_what, float *ring_glimpse, float *ring_score,
                               void *stream) {
    AIR_REQUIRE(what && glimpse && score && valid && state && ring_what && ring_glimpse && ring_score, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRAJ_MAXT && S > 0 && F > 0 && A > 0 && G > 0 && D >= 1, AIR_E_SHAPE);
    AIR_REQUIRE((long)S * F == (long)R && (long)T * R <= (long)INT_MAX && (long)S * D * T <= (long)INT_MAX, AIR_E_SHAPE);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(what) | reinterpret_cast<uintptr_t>(glimpse) | reinterpret_cast<uintptr_t>(score) |
                           reinterpret_cast<uintptr_t>(valid) | reinterpret_cast<uintptr_t>(state) |
                           reinterpret_cast<uintptr_t>(ring_what) | reinterpret_cast<uintptr_t>(ring_glimpse) |
                           reinterpret_cast<uintptr_t>(ring_score);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    TrajStashArgs a = {what, glimpse, score, valid, reinterpret_cast<const int *>(state), ring_what, ring_glimpse, ring_score,
                       T, S, F, R, A, G, D, A % 4 == 0 && air_aligned16(what) && air_aligned16(ring_what),
                       G % 4 == 0 && air_aligned16(glimpse) && air_aligned16(ring_glimpse)};
    const long waves = (long)T * R;
    hipLaunchKernelGGL(track_stash_kernel, dim3((unsigned)air_cdiv(waves, TRAJ_THREADS / 64)), dim3(TRAJ_THREADS), 0,
                       air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

struct TrajFillStreamArgs {
    const float *ring_what, *ring_glimpse, *ring_score;
    const signed char *state;
    const int *src_frame, *src_slot;
    float *out_what, *out_glimpse, *out_score;
    int T, D, C, N, per_seq, A, G, what_vec, glimpse_vec;
};

// air_track_fill with the ring as its source: src_frame is a GLOBAL frame, found at src_frame mod D
__global__ __launch_bounds__(TRAJ_THREADS) void track_fill_stream_kernel(TrajFillStreamArgs a) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * (TRAJ_THREADS / 64) + wid;
    if (e >= (long)a.C * a.N) return;
    const int n = (int)(e % a.N);
    const int s = n / a.per_seq;
    const int st = (int)a.state[e], sf = a.src_frame[e], sj = a.src_slot[e];
    const bool has = st != TRAJ_ABSENT && sf >= 0 && sj >= 0 && sj < a.T;
    const size_t from = has ? ((size_t)s * a.D + sf % a.D) * a.T + sj : 0;
    copy_row_bits_or_zero(has ? a.ring_what + from * a.A : nullptr, a.out_what + (size_t)e * a.A, a.A, a.what_vec != 0, lane);
    copy_row_bits_or_zero(has ? a.ring_glimpse + from * a.G : nullptr, a.out_glimpse + (size_t)e * a.G, a.G, a.glimpse_vec != 0, lane);
    if (lane == 0) reinterpret_cast<unsigned *>(a.out_score)[e] = has ? reinterpret_cast<const unsigned *>(a.ring_score)[from] : 0u;
}

extern "C" int air_track_fill_stream(const float *ring_what, const float *ring_glimpse, const float *ring_score, const signed char *state,
                                     const int *src_frame, const int *src_slot, int T, int S, int D, int C, int N, int per_seq, int A,
                                     int G, float *out_what, float *out_glimpse, float *out_score, void *stream) {
    AIR_REQUIRE(ring_what && ring_glimpse && ring_score && state && src_frame && src_slot && out_what && out_glimpse && out_score,
                AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRAJ_MAXT && C >= 1 && C <= TRAJ_MAXT && S > 0 && D >= 1 && N > 0 && per_seq > 0 && A > 0 && G > 0,
                AIR_E_SHAPE);
    AIR_REQUIRE(N % per_seq == 0 && N / per_seq == S, AIR_E_SHAPE);
    AIR_REQUIRE((long)C * N <= (long)INT_MAX && (long)S * D * T <= (long)INT_MAX, AIR_E_SHAPE);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(ring_what) | reinterpret_cast<uintptr_t>(ring_glimpse) |
                           reinterpret_cast<uintptr_t>(ring_score) | reinterpret_cast<uintptr_t>(src_frame) |
                           reinterpret_cast<uintptr_t>(src_slot) | reinterpret_cast<uintptr_t>(out_what) |
                           reinterpret_cast<uintptr_t>(out_glimpse) | reinterpret_cast<uintptr_t>(out_score);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    TrajFillStreamArgs a = {ring_what, ring_glimpse, ring_score, state, src_frame, src_slot, out_what, out_glimpse, out_score,
                            T, D, C, N, per_seq, A, G, A % 4 == 0 && air_aligned16(ring_what) && air_aligned16(out_what),
                            G % 4 == 0 && air_aligned16(ring_glimpse) && air_aligned16(out_glimpse)};
    const long waves = (long)C * N;
    hipLaunchKernelGGL(track_fill_stream_kernel, dim3((unsigned)air_cdiv(waves, TRAJ_THREADS / 64)), dim3(TRAJ_THREADS), 0,
                       air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
