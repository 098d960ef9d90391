// Tracking objects across the frames of a sequence for gfx950: per-frame parses in, identities out.
//   air_track_associate: per sequence the frames walked in order INSIDE the kernel; a table of at most 32 live tracks, the float64
//                        affinity of every (track, object) pair, greedy matching by a workgroup arg-max, births, ageing;
//   air_track_associate_stream: the same per-frame code on a CHUNK of a stream: the track table is loaded from and stored to a state
//                        that outlives the launch, the frames are numbered globally, the retired tracks come as a list;
//   air_track_score_stream: air_track_score with its map, its per-slot counts, its counters and its IoU sum carried in a state;
//   air_track_associate_motion: the same kernel (either matching) with a per-track Kalman filter: every pair is gated and ranked by the
//                        IoU with the box the track is PREDICTED to have, and a match or a birth advances or starts the filter;
//   air_track_associate_motion_gated: the motion kernel with the pair rule replaced: every pair is gated by its squared Mahalanobis
//                        distance from the filter's predicted state (mean AND covariance) and ranked by 1 / (1 + that distance);
//   air_track_associate_optimal: the same kernel with step 3 replaced: the assignment of the largest summed int64 profit, by a
//                        shortest-augmenting-path Hungarian that one wavefront runs (lane = column);
//   air_track_owner:     the parse's owner maps relabelled from step to track id (int8 in, int16 out): a streaming pass;
//   air_track_score:     CLEAR-MOT counts of the tracks against ground truth whose slot g is one object over a sequence;
//   air_track_idf:       the IDF1 counts of the same tracks: the (ground-truth slot, id) overlap table of a sequence and the largest
//                        one-to-one sum over it, by dynamic programming over the subsets of slots.
//   air_track_hota:      the HOTA counts of the same tracks at 19 localisation thresholds: two passes over the frames, the potential
//                        table of every (slot, id) first, then one optimal matching per frame scored by it (the one-wavefront solver).
//   air_track_mots:      the MOTS counts of the same tracks as MASKS: from the pixel counts air_score_contingency writes for (step
//                        owner map, ground-truth instance map), mask IoU > 1/2 decided in int64, one wavefront per sequence;
//   air_track_stitch:    track fragments joined across long occlusions: per track its own Kalman filter, per (ended, begun later)
//                        pair the Mahalanobis distance of the later track's first sighting from the earlier one's prediction and the
//                        msd of their `what` rows, one optimal assignment over the tracks (the one-wavefront solver), ids relabelled.
// Everything a float decides is float64 with contraction off; no floating-point atomics, no cross-workgroup traffic, one fixed order:
// the same bits run to run.
#include <math.h>
#include <limits.h>
#include <type_traits>
#include "scene_device.h"
#include "traj_device.h"

#define TRACK_THREADS 256
#define TRACK_MAXT 32                    // PARSE_MAXT / SCORE_MAXT: objects per frame, and live tracks per sequence
#define TRACK_MAXG 8                     // SCORE_MAXG
#define TRACK_MAX_IDS 32767              // F * T: an id fits the int16 of track_owner

enum { TRACK_ABSENT = 0, TRACK_MATCHED = 1, TRACK_BORN = 2, TRACK_UNCONFIRMED = 3, TRACK_OVERFLOW = 4, TRACK_NONFINITE = 5 };

__device__ __forceinline__ bool track_finite4(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }

// the better of two (value, key, position) candidates: the larger value, the lower key between equal values.  A candidate that is
// no candidate carries value -1, key INT_MAX, position -1; a NaN is never stored as a value.
__device__ __forceinline__ void track_take_better(double &v, int &key, int &pos, double ov, int okey, int opos) {
    if (ov > v || (ov == v && okey < key)) {
        v = ov;
        key = okey;
        pos = opos;
    }
}
__device__ __forceinline__ void track_wave_argmax(double &v, int &key, int &pos) {      // valid in every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int okey = __shfl_xor(key, off, 64), opos = __shfl_xor(pos, off, 64);
        track_take_better(v, key, pos, ov, okey, opos);
    }
}

// ============================================================================================================
// associate
// ============================================================================================================
struct TrackAssocArgs {
    const float *what, *boxes, *score;
    const int *num_objects;
    int *track_id, *prev_frame, *prev_slot, *num_tracks, *track_first, *track_last, *track_length, *track_gaps, *state_counts;
    float *affinity;
    signed char *obj_state;
    double iou_gate, w, birth_score;
    int T, S, F, A, max_age;
};
// a chunk of a stream: the one-shot arguments (num_tracks and the per-id tables unused) and the carried state (include/air_hip.h
// states the layout)
struct TrackStreamArgs : TrackAssocArgs {
    const int *valid;
    int *st_seq, *st_slots;
    float *st_box, *st_what;
    int *num_retired, *retired_id, *retired_first, *retired_last, *retired_length, *retired_gaps;
};
enum { TRACK_ST_LIVE = 0, TRACK_ST_ID, TRACK_ST_AGE, TRACK_ST_LENGTH, TRACK_ST_GAPS, TRACK_ST_FIRST, TRACK_ST_LAST_FRAME,
       TRACK_ST_LAST_SLOT, TRACK_ST_FIELDS };
// motion: the one-shot arguments, the `where` rows, the noise terms of the trajectory filter and the two prediction outputs
struct TrackMotionArgs : TrackAssocArgs {
    const float *where;
    float *pred_where, *pred_boxes;
    double q[2], r, velocity_var;        // q[0]: the shift components tx, ty; q[1]: the scale components sx, sy (TrajSmoothArgs')
    float Wf, Hf;
};
// the filtered state of slot k, value i: mstate_s[i * 32 + k]
enum { TRACK_MS_X = 0, TRACK_MS_V = 4, TRACK_MS_P = 8, TRACK_MS_DOUBLES = 14 };      // class c: TRACK_MS_P + 3 c (xx, xv, vv)
// the Mahalanobis gate: the motion arguments, the gate (a squared distance) and the d2 of every matched pair
struct TrackGateArgs : TrackMotionArgs {
    double gate_d2;
    float *pred_d2;
};
// the PREDICTED state of slot k in this frame, value i: gstate_s[i * 32 + k] -- xp over [sx, tx, sy, ty], s = Pxx- + r per class
enum { TRACK_GS_X = 0, TRACK_GS_S = 4, TRACK_GS_DOUBLES = 6 };     // class 0: the shifts, class 1: the scales (TRAJ_UPDATE's cl)

// d2 of slot k's predicted state and the `where` row w: e = z - xp, ((e0^2 / s1 + e1^2 / s0) + e2^2 / s1) + e3^2 / s0 -- one product
// and one quotient per term, added in the order [sx, tx, sy, ty].  The pair loop and the row's read-out both run it: the same bits.
__device__ __forceinline__ double track_gate_d2(const double *gstate_s, int k, const float4 w) {
#pragma clang fp contract(off)
    const double *gs = gstate_s + k;
    const double s0 = gs[(TRACK_GS_S + 0) * TRACK_MAXT], s1 = gs[(TRACK_GS_S + 1) * TRACK_MAXT];
    const double e0 = (double)w.x - gs[(TRACK_GS_X + 0) * TRACK_MAXT], e1 = (double)w.y - gs[(TRACK_GS_X + 1) * TRACK_MAXT],
                 e2 = (double)w.z - gs[(TRACK_GS_X + 2) * TRACK_MAXT], e3 = (double)w.w - gs[(TRACK_GS_X + 3) * TRACK_MAXT];
    return ((e0 * e0 / s1 + e1 * e1 / s0) + e2 * e2 / s1) + e3 * e3 / s0;
}

// The assignment of the frame's finite objects (rows, inserted in ascending j) to the 64 columns of one wavefront -- column k < 32 is
// track slot k, column 32 + j is "object j stays unmatched" -- that maximises the summed profit: profit_s[k * 32 + j] >= 1 for an
// admissible pair, -1 for a forbidden one, 0 for staying unmatched.  Shortest augmenting paths with potentials (Jonker-Volgenant
// style): u of row `lane`, v / minv / way / used of column `lane`, all int64, so the optimal value is exact; the column that enters
// the tree next is the unused one of the least minv, the lowest column among equal values.  Returns the row assigned to column
// `lane`, -1 for none.  Every lane of the wavefront must call it.
#define TRACK_NO_COLUMN 64               // the virtual column an insertion starts from
__device__ __forceinline__ int track_solve_wave(const long long *profit_s, const int *ostate_s, int n, int lane) {
    long long u = 0, v = 0;
    int row = -1;
    for (int i = 0; i < n; ++i) {
        if (ostate_s[i] != TRACK_UNCONFIRMED) continue;            // wave-uniform: a NONFINITE object takes no part
        long long minv = LLONG_MAX;
        int way = TRACK_NO_COLUMN, j0 = TRACK_NO_COLUMN, i0 = i;
        bool used = false, in_tree = false;                        // column `lane` / row `lane` is on the alternating tree
        for (;;) {
            if (lane == j0) used = true;
            if (lane == i0) in_tree = true;
            const long long u0 = __shfl(u, i0, 64);
            const long long profit = lane < TRACK_MAXT ? profit_s[lane * TRACK_MAXT + i0] : (lane - TRACK_MAXT == i0 ? 0 : -1);
            if (!used && profit >= 0) {
                const long long cur = -profit - u0 - v;
                if (cur < minv) {
                    minv = cur;
                    way = j0;
                }
            }
            long long delta = used ? LLONG_MAX : minv;             // object i0's own column is never forbidden: a finite minimum
            int j1 = lane;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const long long od = __shfl_xor(delta, off, 64);
                const int oj = __shfl_xor(j1, off, 64);
                if (od < delta || (od == delta && oj < j1)) {
                    delta = od;
                    j1 = oj;
                }
            }
            if (in_tree) u += delta;
            if (used) v -= delta;
            else if (minv != LLONG_MAX) minv -= delta;
            j0 = j1;
            i0 = __shfl(row, j0, 64);
            if (i0 < 0) break;                                     // a free column: the path ends here
        }
        for (;;) {                                                 // the rows along the path move one column on
            const int j1 = __shfl(way, j0, 64);
            const int moved = __shfl(row, j1 & 63, 64);
            if (lane == j0) row = j1 == TRACK_NO_COLUMN ? i : moved;
            j0 = j1;
            if (j0 == TRACK_NO_COLUMN) break;
        }
    }
    return row;
}

// One 256-thread workgroup per sequence.  Track slot k and object j < 32; pair p = k * 32 + j, four pairs per thread.  OPTIMAL: step 3
// is track_solve_wave's assignment (wavefront 0 runs it, the other three wait at the barrier), everything else is the same code.
// STREAM: the table comes from and goes back to the state (one global round trip per launch, none per frame), the frames f <
// clip(valid[s], 0, F) are walked under their global index frames_seen + f, a track last sighted before this chunk takes its `what`
// row from the state, and a retired track goes to the chunk's retired list (its place by a ballot over the 32 slots).
// MOTION: slot k carries the FILTERED state of the trajectory filter at its last sighting (14 doubles in LDS, read and written by
// lane k alone); lane k forms the slot's predicted row and box in step 1, the pair loop of step 2 reads that box where it reads the
// last-sighting box otherwise, and in step 5 lane k advances (a matched track: the coasted frames predicted one by one, then the
// update with the new sighting's `where` row) or starts (a born track) its state.  An object with a non-finite `where` value is
// NONFINITE.  The bits of every other output are those of the kernel without MOTION while every track's rate is exactly 0.
// GATED (with MOTION): in step 1 lane k also forms the PREDICTED state of its slot for this frame -- the frames coasted over predicted
// one by one, then one more predict: xp[4] and s = Pxx- + r per class, 6 doubles per slot in LDS, the values step 5 computes again
// when it books a match --; the pair loop gates on d2 <= gate_d2 and ranks by (1 - w) / (1 + d2) + w / (1 + msd), with no box IoU; the
// row's read-out writes float(d2) of the matched pair.  Everything else is the MOTION kernel's.
template <bool OPTIMAL, bool STREAM = false, bool MOTION = false, bool GATED = false>
__global__ __launch_bounds__(TRACK_THREADS) void track_associate_kernel(
    std::conditional_t<STREAM, TrackStreamArgs,
                       std::conditional_t<GATED, TrackGateArgs, std::conditional_t<MOTION, TrackMotionArgs, TrackAssocArgs>>> a) {
#pragma clang fp contract(off)
    static_assert(!(STREAM && MOTION), "the motion state is not carried across the chunks of a stream");
    static_assert(!GATED || MOTION, "the gate reads the covariance of the motion filter");
    static_assert(!(STREAM && GATED), "no gate on a stream: there is no motion state there");
    __shared__ double gstate_s[GATED ? TRACK_GS_DOUBLES * TRACK_MAXT : 1];       // GATED only
    __shared__ double mstate_s[MOTION ? TRACK_MS_DOUBLES * TRACK_MAXT : 1];      // MOTION only, as the three below
    __shared__ float4 owhere_s[MOTION ? TRACK_MAXT : 1];           // the frame's `where` rows
    __shared__ float4 pwhere_s[MOTION ? TRACK_MAXT : 1], pbox_s[MOTION ? TRACK_MAXT : 1];      // the slots' predicted rows and boxes
    __shared__ int omk_s[MOTION ? TRACK_MAXT : 1];                 // the slot a matched object was matched to
    __shared__ double aff_s[TRACK_MAXT * TRACK_MAXT];              // aff of an admissible pair still open, -1 otherwise
    __shared__ long long profit_s[OPTIMAL ? TRACK_MAXT * TRACK_MAXT : 1];      // OPTIMAL: 1 + floor(aff 2^32), -1 for a forbidden pair
    __shared__ float4 obox_s[TRACK_MAXT], tbox_s[TRACK_MAXT];      // the frame's boxes; the tracks' last-sighting boxes
    __shared__ float oscore_s[TRACK_MAXT], oaff_s[TRACK_MAXT];
    __shared__ int ostate_s[TRACK_MAXT], oid_s[TRACK_MAXT], opf_s[TRACK_MAXT], ops_s[TRACK_MAXT];
    __shared__ int t_live[TRACK_MAXT], t_id[TRACK_MAXT], t_f[TRACK_MAXT], t_j[TRACK_MAXT], t_age[TRACK_MAXT], t_len[TRACK_MAXT],
        t_gaps[TRACK_MAXT];
    __shared__ double wave_v[TRACK_THREADS / 64];
    __shared__ int wave_key[TRACK_THREADS / 64], wave_pos[TRACK_THREADS / 64];
    __shared__ int counts_s[6], next_id_s, nonfinite_s[TRACK_MAXT];
    __shared__ int t_first[STREAM ? TRACK_MAXT : 1], nret_s[1];   // STREAM only
    const int T = a.T, F = a.F, A = a.A, R = a.S * F, FT = F * T;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int base = 0, V = F, n_ret = 0;                                // STREAM: frames_seen, the valid frames, retired so far (tid < 32's)
    if constexpr (STREAM) {
        base = a.st_seq[2 * s];
        const int v = a.valid[s];
        V = v < 0 ? 0 : (v > F ? F : v);
    }
    if (tid < TRACK_MAXT) {
        if constexpr (STREAM) {                                    // the table of the launch before: independent loads, one round trip
            const int *sl = a.st_slots + (size_t)s * TRACK_ST_FIELDS * TRACK_MAXT + tid;
            const int live = sl[TRACK_ST_LIVE * TRACK_MAXT], id = sl[TRACK_ST_ID * TRACK_MAXT], age = sl[TRACK_ST_AGE * TRACK_MAXT],
                      len = sl[TRACK_ST_LENGTH * TRACK_MAXT], gaps = sl[TRACK_ST_GAPS * TRACK_MAXT],
                      first = sl[TRACK_ST_FIRST * TRACK_MAXT], lf = sl[TRACK_ST_LAST_FRAME * TRACK_MAXT],
                      lj = sl[TRACK_ST_LAST_SLOT * TRACK_MAXT];
            const float4 box = *reinterpret_cast<const float4 *>(a.st_box + 4 * ((size_t)s * TRACK_MAXT + tid));
            t_live[tid] = live, t_id[tid] = id, t_age[tid] = age, t_len[tid] = len, t_gaps[tid] = gaps, t_first[tid] = first;
            t_f[tid] = lf, t_j[tid] = lj, tbox_s[tid] = box;
        } else {
            t_live[tid] = 0;
        }
        nonfinite_s[tid] = 0;
    }
    if (tid < 6) counts_s[tid] = 0;
    if (tid == 0) {
        if constexpr (STREAM) next_id_s = a.st_seq[2 * s + 1];
        else next_id_s = 0;
    }
    __syncthreads();

    for (int f = 0; f < V; ++f) {
        const int r = s * F + f;
        const int fg = STREAM ? base + f : f;                      // the frame's index in the stream
        int n = a.num_objects[r];
        n = n < 0 ? 0 : (n > T ? T : n);
        // ---- 1. object states: the boxes and scores by the first threads, the T x A `what` values by the whole workgroup ----------------
        if (tid < TRACK_MAXT) {
            const int j = tid;
            float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
            float sc = 0.f;
            if (j < n) {
                const size_t row = (size_t)j * R + r;
                box = *reinterpret_cast<const float4 *>(a.boxes + 4 * row);
                sc = a.score[row];
            }
            obox_s[j] = box;
            oscore_s[j] = sc;
            oid_s[j] = -1;
            opf_s[j] = -1;
            ops_s[j] = -1;
            oaff_s[j] = 0.f;
            if constexpr (MOTION) {
                float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < n) w4 = *reinterpret_cast<const float4 *>(a.where + 4 * ((size_t)j * R + r));
                owhere_s[j] = w4;
                omk_s[j] = -1;
                if (!track_finite4(w4)) nonfinite_s[j] = 1;        // (every writer writes 1)
                // slot k = tid: where the track is predicted to be m frames after its last sighting -- trajectory's forecast row
                // (shifts extrapolated, scales held; one product and one sum in float64, rounded once) and its box in fp32
                const int k = tid;
                float4 pw = make_float4(0.f, 0.f, 0.f, 0.f), pb = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t_live[k]) {
                    const double m = (double)(fg - t_f[k]);
                    const double *ms = mstate_s + k;
                    pw = make_float4((float)ms[(TRACK_MS_X + 0) * TRACK_MAXT],
                                     (float)(ms[(TRACK_MS_X + 1) * TRACK_MAXT] + m * ms[(TRACK_MS_V + 1) * TRACK_MAXT]),
                                     (float)ms[(TRACK_MS_X + 2) * TRACK_MAXT],
                                     (float)(ms[(TRACK_MS_X + 3) * TRACK_MAXT] + m * ms[(TRACK_MS_V + 3) * TRACK_MAXT]));
                    pb = attention_box4(pw, a.Wf, a.Hf);
                    if (!track_finite4(pb)) pb = tbox_s[k];        // a prediction that leaves fp32: the last-sighting box
                    if constexpr (GATED) {                         // the predicted state m frames on, by the statements of step 5
                        const double q2[2] = {0.5 * a.q[0], 0.5 * a.q[1]}, q4[2] = {0.25 * a.q[0], 0.25 * a.q[1]};
                        double x[4], v[4];
                        TrajCov P[2];
#pragma unroll
                        for (int c = 0; c < 4; ++c) x[c] = ms[(TRACK_MS_X + c) * TRACK_MAXT], v[c] = ms[(TRACK_MS_V + c) * TRACK_MAXT];
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            P[c].xx = ms[(TRACK_MS_P + 3 * c) * TRACK_MAXT];
                            P[c].xv = ms[(TRACK_MS_P + 3 * c + 1) * TRACK_MAXT];
                            P[c].vv = ms[(TRACK_MS_P + 3 * c + 2) * TRACK_MAXT];
                        }
                        const int mi = fg - t_f[k];                // 1 .. max_age + 1
                        for (int i = 1; i < mi; ++i) {
#pragma unroll
                            for (int c = 0; c < 2; ++c) P[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                            for (int c = 0; c < 4; ++c) x[c] = x[c] + v[c];
                        }
                        double *gs = gstate_s + k;
#pragma unroll
                        for (int c = 0; c < 4; ++c) gs[(TRACK_GS_X + c) * TRACK_MAXT] = x[c] + v[c];
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            gs[(TRACK_GS_S + c) * TRACK_MAXT] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]).xx + a.r;
                    }
                }
                pwhere_s[k] = pw;
                pbox_s[k] = pb;
            }
        }
        for (int e = tid; e < n * A; e += TRACK_THREADS) {
            const int j = e / A, q = e - j * A;
            if (!isfinite(a.what[((size_t)j * R + r) * A + q])) nonfinite_s[j] = 1;      // (every writer writes 1)
        }
        __syncthreads();
        // ---- 2. affinity -----------------------------------------------------------------------------------------------------------
        if (tid < TRACK_MAXT) {
            const int j = tid;
            const bool finite = track_finite4(obox_s[j]) && isfinite(oscore_s[j]) && !nonfinite_s[j];
            ostate_s[j] = j < n ? (finite ? TRACK_UNCONFIRMED : TRACK_NONFINITE) : TRACK_ABSENT;      // (finite and open: settled below)
        }
        for (int p = tid; p < TRACK_MAXT * TRACK_MAXT; p += TRACK_THREADS) {
            const int k = p >> 5, j = p & 31;
            double val = -1.0;
            if (t_live[k] && j < n && track_finite4(obox_s[j]) && isfinite(oscore_s[j]) && !nonfinite_s[j]) {
                double iou;                                        // GATED: d2 in its place
                if constexpr (GATED) iou = track_gate_d2(gstate_s, k, owhere_s[j]);
                else if constexpr (MOTION) iou = box_iou_f64(pbox_s[k], obox_s[j]);
                else iou = box_iou_f64(tbox_s[k], obox_s[j]);
                const float *wk;
                if constexpr (STREAM) {                            // sighted in this chunk: in place; before it: the state's copy
                    const int lf = t_f[k] - base;
                    wk = lf >= 0 ? a.what + ((size_t)t_j[k] * R + (size_t)s * F + lf) * A
                                 : a.st_what + ((size_t)s * TRACK_MAXT + k) * A;
                } else {
                    wk = a.what + ((size_t)t_j[k] * R + (size_t)s * F + t_f[k]) * A;      // read in place
                }
                const float *wj = a.what + ((size_t)j * R + r) * A;
                double sum = 0.0;
                int q = 0;
                for (; q + 8 <= A; q += 8) {                       // eight loads of each row in flight, added in ascending a
                    float x[8], y[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        x[u] = wk[q + u];
                        y[u] = wj[q + u];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const double d = (double)x[u] - (double)y[u];
                        sum = sum + d * d;
                    }
                }
                for (; q < A; ++q) {
                    const double d = (double)wk[q] - (double)wj[q];
                    sum = sum + d * d;
                }
                const double msd = sum / (double)A;
                if constexpr (GATED) {                             // (a NaN or an inf fails the gate; iou_gate is not applied)
                    const double aff = (1.0 - a.w) / (1.0 + iou) + a.w / (1.0 + msd);
                    if (iou <= a.gate_d2) val = aff;
                } else {
                    const double aff = (1.0 - a.w) * iou + a.w / (1.0 + msd);
                    if (iou > a.iou_gate) val = aff;
                }
            }
            aff_s[p] = val;
            if constexpr (OPTIMAL) profit_s[p] = val >= 0.0 ? 1 + (long long)floor(val * 4294967296.0) : -1;      // (exact: a power of two)
        }
        __syncthreads();
        // ---- 3. matching: the optimal assignment, or greedily ---------------------------------------------------------------------------
        if constexpr (OPTIMAL) {
            if (wid == 0) {
                const int j = track_solve_wave(profit_s, ostate_s, n, lane);
                if (lane < TRACK_MAXT && j >= 0) {                  // the pairs share neither a track nor an object: any order
                    const int k = lane;
                    ostate_s[j] = TRACK_MATCHED;
                    oid_s[j] = t_id[k];
                    opf_s[j] = t_f[k];
                    ops_s[j] = t_j[k];
                    oaff_s[j] = (float)aff_s[k * TRACK_MAXT + j];
                    if constexpr (MOTION) omk_s[j] = k;
                    t_gaps[k] += t_age[k] > 0 ? 1 : 0;
                    t_age[k] = 0;
                    t_len[k] += 1;
                    t_f[k] = fg;
                    t_j[k] = j;
                    tbox_s[k] = obox_s[j];
                }
            }
            __syncthreads();
        }
        while (!OPTIMAL) {                                         // (a compile-time constant: no greedy round in the optimal kernel)
            double v = -1.0;
            int key = INT_MAX, pos = -1;
#pragma unroll
            for (int q = 0; q < TRACK_MAXT * TRACK_MAXT / TRACK_THREADS; ++q) {
                const int p = tid + q * TRACK_THREADS;
                const double x = aff_s[p];
                if (x >= 0.0) track_take_better(v, key, pos, x, t_id[p >> 5] * TRACK_MAXT + (p & 31), p);
            }
            track_wave_argmax(v, key, pos);
            if (lane == 0) {
                wave_v[wid] = v;
                wave_key[wid] = key;
                wave_pos[wid] = pos;
            }
            __syncthreads();
            v = wave_v[0], key = wave_key[0], pos = wave_pos[0];
#pragma unroll
            for (int q = 1; q < TRACK_THREADS / 64; ++q) track_take_better(v, key, pos, wave_v[q], wave_key[q], wave_pos[q]);
            if (pos < 0) break;                                    // workgroup-uniform
            const int k = pos >> 5, j = pos & 31;
            if (tid == 0) {
                ostate_s[j] = TRACK_MATCHED;
                oid_s[j] = t_id[k];
                opf_s[j] = t_f[k];
                ops_s[j] = t_j[k];
                oaff_s[j] = (float)v;
                if constexpr (MOTION) omk_s[j] = k;
                t_gaps[k] += t_age[k] > 0 ? 1 : 0;
                t_age[k] = 0;
                t_len[k] += 1;
                t_f[k] = fg;
                t_j[k] = j;
                tbox_s[k] = obox_s[j];
            }
            if (tid < TRACK_MAXT) {
                aff_s[k * TRACK_MAXT + tid] = -1.0;
                aff_s[tid * TRACK_MAXT + j] = -1.0;
            }
            __syncthreads();
        }
        // ---- 4. births ----------------------------------------------------------------------------------------------------------------
        if (tid == 0) {
            int next_id = next_id_s;
            for (int j = 0; j < n; ++j) {
                if (ostate_s[j] != TRACK_UNCONFIRMED || !((double)oscore_s[j] >= a.birth_score)) continue;
                int k = 0;
                while (k < TRACK_MAXT && t_live[k]) ++k;
                if (k == TRACK_MAXT || (STREAM && next_id >= TRACK_MAX_IDS)) {      // STREAM: the ids of a stream are 0..32766
                    ostate_s[j] = TRACK_OVERFLOW;
                    continue;
                }
                ostate_s[j] = TRACK_BORN;
                oid_s[j] = next_id;
                t_live[k] = 1;
                t_id[k] = next_id;
                t_f[k] = fg;
                t_j[k] = j;
                t_age[k] = 0;
                t_len[k] = 1;
                t_gaps[k] = 0;
                tbox_s[k] = obox_s[j];
                if constexpr (STREAM) t_first[k] = fg;
                else a.track_first[(size_t)s * FT + next_id] = f;   // next_id < F * T: one id per object at most
                ++next_id;
            }
            next_id_s = next_id;
        }
        __syncthreads();
        // ---- 5. ageing, and the frame's rows -------------------------------------------------------------------------------------------
        if (tid < TRACK_MAXT) {
            const int k = tid;
            nonfinite_s[k] = 0;                                     // (for the next frame: read last in step 2)
            bool retire = false;
            if (t_live[k] && t_f[k] != fg) {
                t_age[k] += 1;
                if (t_age[k] > a.max_age) {
                    if constexpr (STREAM) {
                        retire = true;
                    } else {
                        const size_t at = (size_t)s * FT + t_id[k];
                        a.track_last[at] = t_f[k];
                        a.track_length[at] = t_len[k];
                        a.track_gaps[at] = t_gaps[k];
                        t_live[k] = 0;
                    }
                }
            }
            if constexpr (MOTION) {                                // the filter state of a slot sighted in this frame: lane = slot
                if (t_live[k] && t_f[k] == fg) {
                    const int j = t_j[k];
                    const float4 w4 = owhere_s[j];
                    const double z[4] = {(double)w4.x, (double)w4.y, (double)w4.z, (double)w4.w};
                    double *ms = mstate_s + k;
                    double x[4], v[4];
                    TrajCov P[2];
                    if (ostate_s[j] == TRACK_BORN) {               // start: x = z, v = 0, P = (r, 0, velocity_var)
#pragma unroll
                        for (int c = 0; c < 4; ++c) x[c] = z[c], v[c] = 0.0;
                        P[0].xx = P[1].xx = a.r;
                        P[0].xv = P[1].xv = 0.0;
                        P[0].vv = P[1].vv = a.velocity_var;
                    } else {                                       // matched: the frames coasted over one by one, then the update
                        const double q2[2] = {0.5 * a.q[0], 0.5 * a.q[1]}, q4[2] = {0.25 * a.q[0], 0.25 * a.q[1]};
#pragma unroll
                        for (int c = 0; c < 4; ++c) x[c] = ms[(TRACK_MS_X + c) * TRACK_MAXT], v[c] = ms[(TRACK_MS_V + c) * TRACK_MAXT];
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            P[c].xx = ms[(TRACK_MS_P + 3 * c) * TRACK_MAXT];
                            P[c].xv = ms[(TRACK_MS_P + 3 * c + 1) * TRACK_MAXT];
                            P[c].vv = ms[(TRACK_MS_P + 3 * c + 2) * TRACK_MAXT];
                        }
                        const int m = fg - opf_s[j];               // 1 .. max_age + 1
                        for (int i = 1; i < m; ++i) {
#pragma unroll
                            for (int c = 0; c < 2; ++c) P[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                            for (int c = 0; c < 4; ++c) x[c] = x[c] + v[c];
                        }
                        TrajCov Pp[2];
                        double xp[4], vp[4];
#pragma unroll
                        for (int c = 0; c < 2; ++c) Pp[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) xp[c] = x[c] + v[c], vp[c] = v[c];
                        TRAJ_UPDATE(P, Pp, x, v, xp, vp, z, a.r)
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) ms[(TRACK_MS_X + c) * TRACK_MAXT] = x[c], ms[(TRACK_MS_V + c) * TRACK_MAXT] = v[c];
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        ms[(TRACK_MS_P + 3 * c) * TRACK_MAXT] = P[c].xx;
                        ms[(TRACK_MS_P + 3 * c + 1) * TRACK_MAXT] = P[c].xv;
                        ms[(TRACK_MS_P + 3 * c + 2) * TRACK_MAXT] = P[c].vv;
                    }
                }
            }
            if constexpr (STREAM) {                                // the retired list: ascending frame, then ascending slot
                const unsigned long long retiring = __ballot(retire);      // (the 32 threads of this branch are lanes 0..31 of one wavefront)
                if (retire) {
                    const size_t at = (size_t)s * (TRACK_MAXT + FT) + n_ret + __popcll(retiring & ((1ull << k) - 1ull));
                    a.retired_id[at] = t_id[k];
                    a.retired_first[at] = t_first[k];
                    a.retired_last[at] = t_f[k];
                    a.retired_length[at] = t_len[k];
                    a.retired_gaps[at] = t_gaps[k];
                    t_live[k] = 0;
                }
                n_ret += __popcll(retiring);
            }
            if (tid < T) {
                const size_t row = (size_t)tid * R + r;
                const int state = ostate_s[tid];
                a.track_id[row] = oid_s[tid];
                a.obj_state[row] = (signed char)state;
                a.affinity[row] = oaff_s[tid];
                a.prev_frame[row] = opf_s[tid];
                a.prev_slot[row] = ops_s[tid];
                if constexpr (MOTION) {                            // the prediction the match was made against; zero unless matched
                    const int mk = omk_s[tid];
                    float4 pw = pwhere_s[mk < 0 ? 0 : mk], pb = pbox_s[mk < 0 ? 0 : mk];      // (a select of values, not of addresses)
                    if (mk < 0) pw = pb = make_float4(0.f, 0.f, 0.f, 0.f);
                    reinterpret_cast<float4 *>(a.pred_where)[row] = pw;
                    reinterpret_cast<float4 *>(a.pred_boxes)[row] = pb;
                    if constexpr (GATED) {                         // (gstate_s[mk] is this frame's: a matched slot stays its track's)
                        float d2 = 0.f;
                        if (mk >= 0) d2 = (float)track_gate_d2(gstate_s, mk, owhere_s[tid]);
                        a.pred_d2[row] = d2;
                    }
                }
                atomicAdd(&counts_s[state], 1);                    // integer adds in LDS: the order does not matter
            }
        }
        __syncthreads();
    }
    if constexpr (STREAM) {
        // ---- the padding rows, the state, the unused rows of the retired list, the counts ---------------------------------------------
        const int cap = TRACK_MAXT + FT;
        if (tid == 0) nret_s[0] = n_ret;
        for (int e = tid; e < (F - V) * T; e += TRACK_THREADS) {
            const int fp = e / T, j = e - fp * T;
            const size_t row = (size_t)j * R + (size_t)s * F + V + fp;
            a.track_id[row] = -1;
            a.obj_state[row] = (signed char)TRACK_ABSENT;
            a.affinity[row] = 0.f;
            a.prev_frame[row] = -1;
            a.prev_slot[row] = -1;
        }
        if (tid < TRACK_MAXT) {                                    // a slot that is not live is stored in one canonical form
            int *sl = a.st_slots + (size_t)s * TRACK_ST_FIELDS * TRACK_MAXT + tid;
            const bool live = t_live[tid] != 0;
            sl[TRACK_ST_LIVE * TRACK_MAXT] = live ? 1 : 0;
            sl[TRACK_ST_ID * TRACK_MAXT] = live ? t_id[tid] : -1;
            sl[TRACK_ST_AGE * TRACK_MAXT] = live ? t_age[tid] : 0;
            sl[TRACK_ST_LENGTH * TRACK_MAXT] = live ? t_len[tid] : 0;
            sl[TRACK_ST_GAPS * TRACK_MAXT] = live ? t_gaps[tid] : 0;
            sl[TRACK_ST_FIRST * TRACK_MAXT] = live ? t_first[tid] : -1;
            sl[TRACK_ST_LAST_FRAME * TRACK_MAXT] = live ? t_f[tid] : -1;
            sl[TRACK_ST_LAST_SLOT * TRACK_MAXT] = live ? t_j[tid] : -1;
            *reinterpret_cast<float4 *>(a.st_box + 4 * ((size_t)s * TRACK_MAXT + tid)) = live ? tbox_s[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // the `what` rows of the tracks sighted in this chunk: a bit copy, eight values per thread loaded before the first is stored
        // (the stores may alias the loads for all the compiler knows: one global round trip per batch, not one per value)
        for (int e0 = tid; e0 < TRACK_MAXT * A; e0 += 8 * TRACK_THREADS) {
            float v[8];
            int act[8];                                            // 0: leave the state's row, 1: store v
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * TRACK_THREADS;
                v[u] = 0.f;
                act[u] = 0;
                if (e < TRACK_MAXT * A) {
                    const int k = e / A, q = e - k * A;
                    act[u] = !t_live[k] || t_f[k] >= base;
                    if (t_live[k] && t_f[k] >= base) v[u] = a.what[((size_t)t_j[k] * R + (size_t)s * F + (t_f[k] - base)) * A + q];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (act[u]) a.st_what[(size_t)s * TRACK_MAXT * A + e0 + u * TRACK_THREADS] = v[u];
        }
        if (tid == 0) {
            a.st_seq[2 * s] = base + V;
            a.st_seq[2 * s + 1] = next_id_s;
        }
        __syncthreads();
        const int nr = nret_s[0];
        for (int i = nr + tid; i < cap; i += TRACK_THREADS) {
            const size_t at = (size_t)s * cap + i;
            a.retired_id[at] = -1;
            a.retired_first[at] = -1;
            a.retired_last[at] = -1;
            a.retired_length[at] = 0;
            a.retired_gaps[at] = 0;
        }
        if (tid == 0) a.num_retired[s] = nr;
        if (tid < 6) a.state_counts[(size_t)s * 6 + tid] = counts_s[tid];
        return;
    }
    // ---- the tracks alive at the end, the unused rows of the track tables, the counts -------------------------------------------------
    if (tid < TRACK_MAXT && t_live[tid]) {
        const size_t at = (size_t)s * FT + t_id[tid];
        a.track_last[at] = t_f[tid];
        a.track_length[at] = t_len[tid];
        a.track_gaps[at] = t_gaps[tid];
    }
    const int issued = next_id_s;
    for (int i = issued + tid; i < FT; i += TRACK_THREADS) {
        const size_t at = (size_t)s * FT + i;
        a.track_first[at] = -1;
        a.track_last[at] = -1;
        a.track_length[at] = 0;
        a.track_gaps[at] = 0;
    }
    if (tid == 0) a.num_tracks[s] = issued;
    if (tid < 6) a.state_counts[(size_t)s * 6 + tid] = counts_s[tid];
}

// ---- the host side of the association entries ------------------------------------------------------------------------------------
// the arguments every entry has, from the prototypes' order into the kernel's struct (a stream has no per-id tables: nullptr)
static TrackAssocArgs track_assoc_args(const float *what, const float *boxes, const float *score, const int *num_objects, int T, int S,
                                       int F, int A, double iou_gate, double appearance_weight, double birth_score, int max_age,
                                       int *track_id, signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot,
                                       int *num_tracks, int *track_first, int *track_last, int *track_length, int *track_gaps,
                                       int *state_counts) {
    return {what, boxes, score, num_objects, track_id, prev_frame, prev_slot, num_tracks, track_first, track_last, track_length,
            track_gaps, state_counts, affinity, obj_state, iou_gate, appearance_weight, birth_score, T, S, F, A, max_age};
}

static bool track_aligned4(std::initializer_list<const void *> pointers) {
    uintptr_t bits = 0;
    for (const void *q : pointers) bits |= reinterpret_cast<uintptr_t>(q);
    return (bits & 3u) == 0;
}

// The checks every entry makes of those arguments, one status after the other: NULL, SHAPE, ALIGN.  `st`: a chunk of a stream, which
// has its state and retired lists where a one-shot call has the per-id tables, and `matching` as an argument; its own checks stand
// where the stream entry has always made them, so an input with several faults returns the status it always returned.
static int track_associate_check(const TrackAssocArgs &a, int R, const TrackStreamArgs *st = nullptr, int matching = 0) {
    AIR_REQUIRE(a.what && a.boxes && a.score && a.num_objects && a.track_id && a.obj_state && a.affinity && a.prev_frame &&
                a.prev_slot && a.state_counts, AIR_E_NULL);
    AIR_REQUIRE(st ? st->valid && st->st_seq && st->st_slots && st->st_box && st->st_what && st->num_retired && st->retired_id &&
                     st->retired_first && st->retired_last && st->retired_length && st->retired_gaps
                   : a.num_tracks && a.track_first && a.track_last && a.track_length && a.track_gaps, AIR_E_NULL);
    AIR_REQUIRE(a.T >= 1 && a.T <= TRACK_MAXT && a.S > 0 && a.F > 0 && a.A > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)a.F * a.T <= TRACK_MAX_IDS && (long)a.S * a.F == (long)R && (long)a.S * a.F * a.T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(a.iou_gate >= 0.0 && a.iou_gate < 1.0 && a.w >= 0.0 && a.w <= 1.0, AIR_E_SHAPE);
    AIR_REQUIRE(a.birth_score >= 0.0 && a.birth_score <= 1.0 && a.max_age >= 0, AIR_E_SHAPE);
    if (st) {
        AIR_REQUIRE(matching == 0 || matching == 1, AIR_E_SHAPE);
        AIR_REQUIRE((long)a.S * TRACK_MAXT * a.A <= (long)INT_MAX, AIR_E_SHAPE);
    }
    AIR_REQUIRE(air_aligned16(a.boxes) && (!st || air_aligned16(st->st_box)), AIR_E_ALIGN);
    AIR_REQUIRE(track_aligned4({a.what, a.score, a.num_objects, a.track_id, a.affinity, a.prev_frame, a.prev_slot, a.num_tracks,
                                a.track_first, a.track_last, a.track_length, a.track_gaps, a.state_counts}), AIR_E_ALIGN);
    if (st)
        AIR_REQUIRE(track_aligned4({st->valid, st->st_seq, st->st_slots, st->st_what, st->num_retired, st->retired_id, st->retired_first,
                                    st->retired_last, st->retired_length, st->retired_gaps}), AIR_E_ALIGN);
    return AIR_OK;
}

// the checks and the one dispatch: the kernel's template flags are the kind of its argument struct and the matching
template <class Args>
static int track_associate_launch(bool optimal, const Args &a, int R, void *stream, const TrackStreamArgs *st = nullptr, int matching = 0) {
    constexpr bool STREAM = std::is_same_v<Args, TrackStreamArgs>, MOTION = std::is_base_of_v<TrackMotionArgs, Args>,
                   GATED = std::is_same_v<Args, TrackGateArgs>;
    const int status = track_associate_check(a, R, st, matching);
    if (status != AIR_OK) return status;
    if (optimal)
        hipLaunchKernelGGL((track_associate_kernel<true, STREAM, MOTION, GATED>), dim3((unsigned)a.S), dim3(TRACK_THREADS), 0,
                           air_stream(stream), a);
    else
        hipLaunchKernelGGL((track_associate_kernel<false, STREAM, MOTION, GATED>), dim3((unsigned)a.S), dim3(TRACK_THREADS), 0,
                           air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// The motion entries' own checks and fields, into m.  `pred_d2`: the gated entry's, whose two checks stand where that entry has always
// made them (its gate_d2 and pred_d2 fields are the caller's to set).
static int track_motion_args(TrackMotionArgs &m, const float *where, int H, int W, int matching, double q_shift, double q_scale,
                             double measurement_noise, double velocity_var, float *pred_where, float *pred_boxes, bool gated = false,
                             double gate_d2 = 0.0, const float *pred_d2 = nullptr) {
    AIR_REQUIRE(where && pred_where && pred_boxes && (!gated || pred_d2), AIR_E_NULL);
    AIR_REQUIRE(matching == 0 || matching == 1, AIR_E_SHAPE);
    AIR_REQUIRE(H >= 1 && W >= 1, AIR_E_SHAPE);
    AIR_REQUIRE(traj_noise_check(q_shift, q_scale, measurement_noise, velocity_var) == AIR_OK, AIR_E_SHAPE);
    AIR_REQUIRE(!gated || (isfinite(gate_d2) && gate_d2 > 0.0), AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where) && air_aligned16(pred_where) && air_aligned16(pred_boxes), AIR_E_ALIGN);
    AIR_REQUIRE(track_aligned4({pred_d2}), AIR_E_ALIGN);
    m.where = where, m.pred_where = pred_where, m.pred_boxes = pred_boxes;
    m.q[0] = q_shift, m.q[1] = q_scale, m.r = measurement_noise, m.velocity_var = velocity_var;
    m.Wf = (float)W, m.Hf = (float)H;
    return AIR_OK;
}

extern "C" int air_track_associate(const float *what, const float *boxes, const float *score, const int *num_objects, int T, int S,
                                   int F, int R, int A, double iou_gate, double appearance_weight, double birth_score, int max_age,
                                   int *track_id, signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot,
                                   int *num_tracks, int *track_first, int *track_last, int *track_length, int *track_gaps,
                                   int *state_counts, void *stream) {
    return track_associate_launch(false, track_assoc_args(what, boxes, score, num_objects, T, S, F, A, iou_gate, appearance_weight,
                                                          birth_score, max_age, track_id, obj_state, affinity, prev_frame, prev_slot,
                                                          num_tracks, track_first, track_last, track_length, track_gaps, state_counts),
                                  R, stream);
}

extern "C" int air_track_associate_optimal(const float *what, const float *boxes, const float *score, const int *num_objects, int T,
                                           int S, int F, int R, int A, double iou_gate, double appearance_weight, double birth_score,
                                           int max_age, int *track_id, signed char *obj_state, float *affinity, int *prev_frame,
                                           int *prev_slot, int *num_tracks, int *track_first, int *track_last, int *track_length,
                                           int *track_gaps, int *state_counts, void *stream) {
    return track_associate_launch(true, track_assoc_args(what, boxes, score, num_objects, T, S, F, A, iou_gate, appearance_weight,
                                                         birth_score, max_age, track_id, obj_state, affinity, prev_frame, prev_slot,
                                                         num_tracks, track_first, track_last, track_length, track_gaps, state_counts),
                                  R, stream);
}

extern "C" int air_track_associate_motion(const float *what, const float *where, const float *boxes, const float *score,
                                          const int *num_objects, int T, int S, int F, int R, int A, int H, int W, double iou_gate,
                                          double appearance_weight, double birth_score, int max_age, int matching, double q_shift,
                                          double q_scale, double measurement_noise, double velocity_var, int *track_id,
                                          signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot, int *num_tracks,
                                          int *track_first, int *track_last, int *track_length, int *track_gaps, int *state_counts,
                                          float *pred_where, float *pred_boxes, void *stream) {
    TrackMotionArgs m = {};
    const int status = track_motion_args(m, where, H, W, matching, q_shift, q_scale, measurement_noise, velocity_var, pred_where, pred_boxes);
    if (status != AIR_OK) return status;
    static_cast<TrackAssocArgs &>(m) = track_assoc_args(what, boxes, score, num_objects, T, S, F, A, iou_gate, appearance_weight, birth_score,
                                                        max_age, track_id, obj_state, affinity, prev_frame, prev_slot, num_tracks,
                                                        track_first, track_last, track_length, track_gaps, state_counts);
    return track_associate_launch(matching == 1, m, R, stream);
}

extern "C" int air_track_associate_motion_gated(const float *what, const float *where, const float *boxes, const float *score,
                                                const int *num_objects, int T, int S, int F, int R, int A, int H, int W, double iou_gate,
                                                double appearance_weight, double birth_score, int max_age, int matching, double q_shift,
                                                double q_scale, double measurement_noise, double velocity_var, double gate_d2,
                                                int *track_id, signed char *obj_state, float *affinity, int *prev_frame, int *prev_slot,
                                                int *num_tracks, int *track_first, int *track_last, int *track_length, int *track_gaps,
                                                int *state_counts, float *pred_where, float *pred_boxes, float *pred_d2, void *stream) {
    TrackGateArgs g = {};
    const int status = track_motion_args(g, where, H, W, matching, q_shift, q_scale, measurement_noise, velocity_var, pred_where, pred_boxes,
                                         true, gate_d2, pred_d2);
    if (status != AIR_OK) return status;
    g.gate_d2 = gate_d2, g.pred_d2 = pred_d2;
    static_cast<TrackAssocArgs &>(g) = track_assoc_args(what, boxes, score, num_objects, T, S, F, A, iou_gate, appearance_weight, birth_score,
                                                        max_age, track_id, obj_state, affinity, prev_frame, prev_slot, num_tracks,
                                                        track_first, track_last, track_length, track_gaps, state_counts);
    return track_associate_launch(matching == 1, g, R, stream);
}

extern "C" int air_track_associate_stream(const float *what, const float *boxes, const float *score, const int *num_objects, int T, int S,
                                          int F, int R, int A, double iou_gate, double appearance_weight, double birth_score,
                                          int max_age, const int *valid, int matching, int *st_seq, int *st_slots, float *st_box,
                                          float *st_what, int *track_id, signed char *obj_state, float *affinity, int *prev_frame,
                                          int *prev_slot, int *state_counts, int *num_retired, int *retired_id, int *retired_first,
                                          int *retired_last, int *retired_length, int *retired_gaps, void *stream) {
    TrackStreamArgs a;
    static_cast<TrackAssocArgs &>(a) = track_assoc_args(what, boxes, score, num_objects, T, S, F, A, iou_gate, appearance_weight, birth_score,
                                                        max_age, track_id, obj_state, affinity, prev_frame, prev_slot, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr, state_counts);
    a.valid = valid, a.st_seq = st_seq, a.st_slots = st_slots, a.st_box = st_box, a.st_what = st_what, a.num_retired = num_retired;
    a.retired_id = retired_id, a.retired_first = retired_first, a.retired_last = retired_last, a.retired_length = retired_length;
    a.retired_gaps = retired_gaps;
    return track_associate_launch(matching == 1, a, R, stream, &a, matching);
}

// ============================================================================================================
// owner
// ============================================================================================================
__device__ __forceinline__ unsigned track_owner_pair(unsigned bytes, int shift, const short *lut, int T) {
    const int o0 = (int)(signed char)(bytes >> shift) + 1, o1 = (int)(signed char)(bytes >> (shift + 8)) + 1;
    const unsigned lo = (unsigned short)((unsigned)o0 <= (unsigned)T ? lut[o0] : (short)-1);
    const unsigned hi = (unsigned short)((unsigned)o1 <= (unsigned)T ? lut[o1] : (short)-1);
    return lo | (hi << 16);
}

// One workgroup per image (grid-stride over the images); lut[o + 1] = the track id of step o, lut[0] = -1.  The body of an image is
// read as 16-byte vectors from the first 16-byte boundary of its owner row on and written as two 16-byte (or four 8-byte) vectors
// when the output is aligned to that at the same pixel; the pixels in front of the boundary and behind the last whole vector -- and
// the whole image when the output is aligned to neither -- go one at a time.
__global__ __launch_bounds__(TRACK_THREADS) void track_owner_kernel(const signed char *__restrict__ owner,
                                                                    const int *__restrict__ track_id, int T, int R, int HW,
                                                                    short *__restrict__ out) {
    __shared__ short lut[TRACK_MAXT + 1];
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        if (tid <= T) lut[tid] = tid == 0 ? (short)-1 : (short)track_id[(size_t)(tid - 1) * R + r];
        __syncthreads();
        const signed char *po = owner + (size_t)r * HW;
        short *pt = out + (size_t)r * HW;
        int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(po) & 15u)) & 15u);
        if (head > HW) head = HW;
        const unsigned out_mis = (unsigned)(reinterpret_cast<uintptr_t>(pt + head) & 15u);
        int nvec = (HW - head) >> 4;
        if (out_mis != 0 && out_mis != 8) {                        // every pixel on the word path
            head = HW;
            nvec = 0;
        }
        const int tail0 = head + 16 * nvec;
        const uint4 *vo = reinterpret_cast<const uint4 *>(po + head);
        for (int v = tid; v < nvec; v += TRACK_THREADS) {
            const uint4 b = vo[v];
            const uint4 lo = make_uint4(track_owner_pair(b.x, 0, lut, T), track_owner_pair(b.x, 16, lut, T),
                                        track_owner_pair(b.y, 0, lut, T), track_owner_pair(b.y, 16, lut, T));
            const uint4 hi = make_uint4(track_owner_pair(b.z, 0, lut, T), track_owner_pair(b.z, 16, lut, T),
                                        track_owner_pair(b.w, 0, lut, T), track_owner_pair(b.w, 16, lut, T));
            short *dst = pt + head + 16 * v;
            if (out_mis == 0) {
                reinterpret_cast<uint4 *>(dst)[0] = lo;
                reinterpret_cast<uint4 *>(dst)[1] = hi;
            } else {
                reinterpret_cast<uint2 *>(dst)[0] = make_uint2(lo.x, lo.y);
                reinterpret_cast<uint2 *>(dst)[1] = make_uint2(lo.z, lo.w);
                reinterpret_cast<uint2 *>(dst)[2] = make_uint2(hi.x, hi.y);
                reinterpret_cast<uint2 *>(dst)[3] = make_uint2(hi.z, hi.w);
            }
        }
        const int n_edge = head + (HW - tail0);
        for (int e = tid; e < n_edge; e += TRACK_THREADS) {
            const int p = e < head ? e : tail0 + (e - head);
            const int o = (int)po[p] + 1;
            pt[p] = (unsigned)o <= (unsigned)T ? lut[o] : (short)-1;
        }
        __syncthreads();                                           // the table is rewritten for the next image
    }
}

extern "C" int air_track_owner(const signed char *owner, const int *track_id, int T, int R, int H, int W, short *track_owner,
                               void *stream) {
    AIR_REQUIRE(owner && track_id && track_owner, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && R > 0 && H > 0 && W > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)H * W <= (long)INT_MAX && (long)R * H * W <= (long)INT_MAX && (long)R * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE((reinterpret_cast<uintptr_t>(track_id) & 3u) == 0 && (reinterpret_cast<uintptr_t>(track_owner) & 1u) == 0, AIR_E_ALIGN);
    const int cap = 256 * 16;
    hipLaunchKernelGGL(track_owner_kernel, dim3((unsigned)(R < cap ? R : cap)), dim3(TRACK_THREADS), 0, air_stream(stream), owner,
                       track_id, T, R, H * W, track_owner);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// score
// ============================================================================================================
struct TrackScoreArgs {
    const float *boxes, *gt_boxes;
    const int *num_objects, *track_id;
    int *seq_counts, *gt_match;
    double *seq_iou;
    double tau;
    int T, G, S, F;
};
// a chunk of a stream: st_i [S, 32] = {gt, matches, misses, fp, idsw, 0, 0, 0, map[8], tracked[8], present[8]}, st_f [S] = sum_iou
struct TrackScoreStreamArgs : TrackScoreArgs {
    const int *valid;
    int *st_i;
    double *st_f;
};
#define TRACK_SCORE_ST 32

// One workgroup of one wavefront per sequence.  Pair p = g * 32 + j, four pairs per lane.  STREAM: map, tracked, present, the counters
// and sum_iou continue from the state and go back to it; the frames f < clip(valid[s], 0, F) are walked.
template <bool STREAM> __global__ __launch_bounds__(64) void track_score_kernel(std::conditional_t<STREAM, TrackScoreStreamArgs, TrackScoreArgs> a) {
#pragma clang fp contract(off)
    __shared__ double iou_s[TRACK_MAXG * TRACK_MAXT];
    __shared__ float4 hbox_s[TRACK_MAXT], gbox_s[TRACK_MAXG];
    __shared__ int hid_s[TRACK_MAXT], jused_s[TRACK_MAXT];         // a hypothesis' track id (-1: no hypothesis); taken by a match
    __shared__ int gpresent_s[TRACK_MAXG], gm_s[TRACK_MAXG], cand_s[TRACK_MAXG], map_s[TRACK_MAXG], tracked_s[TRACK_MAXG],
        frames_s[TRACK_MAXG];
    const int T = a.T, G = a.G, F = a.F, R = a.S * F;
    const int s = blockIdx.x, lane = threadIdx.x;
    if constexpr (!STREAM) {
        if (lane < TRACK_MAXG) {
            map_s[lane] = -1;
            tracked_s[lane] = 0;
            frames_s[lane] = 0;
        }
    }
    int n_gt = 0, n_match = 0, n_miss = 0, n_fp = 0, n_idsw = 0;   // lane 0's
    double sum_iou = 0.0;
    int V = F;
    if constexpr (STREAM) {
        const int *c = a.st_i + (size_t)s * TRACK_SCORE_ST;
        const int v = a.valid[s];
        V = v < 0 ? 0 : (v > F ? F : v);
        n_gt = c[0], n_match = c[1], n_miss = c[2], n_fp = c[3], n_idsw = c[4];
        sum_iou = a.st_f[s];
        if (lane < TRACK_MAXG) {
            map_s[lane] = c[8 + lane];
            tracked_s[lane] = c[16 + lane];
            frames_s[lane] = c[24 + lane];
        }
    }
    __syncthreads();
    for (int f = 0; f < V; ++f) {
        const int r = s * F + f;
        int n = a.num_objects[r];
        n = n < 0 ? 0 : (n > T ? T : n);
        if (lane < TRACK_MAXT) {
            const int j = lane;
            float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
            int id = -1;
            if (j < n) {
                const size_t row = (size_t)j * R + r;
                box = *reinterpret_cast<const float4 *>(a.boxes + 4 * row);
                const int t = a.track_id[row];
                if (t >= 0 && track_finite4(box)) id = t;
            }
            hbox_s[j] = box;
            hid_s[j] = id;
            jused_s[j] = 0;
        }
        if (lane < TRACK_MAXG) {
            const int g = lane;
            float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < G) gb = *reinterpret_cast<const float4 *>(a.gt_boxes + 4 * ((size_t)r * G + g));
            gbox_s[g] = gb;
            gpresent_s[g] = (g < G && gb.z > 0.f) ? 1 : 0;
            gm_s[g] = -1;
        }
        __syncthreads();
        for (int p = lane; p < TRACK_MAXG * TRACK_MAXT; p += 64) {
            const int g = p >> 5, j = p & 31;
            iou_s[p] = (gpresent_s[g] && hid_s[j] >= 0) ? box_iou_f64(gbox_s[g], hbox_s[j]) : 0.0;
        }
        __syncthreads();
        // ---- 1. a remembered track that is still on its object keeps it (ascending g; a hypothesis is taken once) -------------------
        if (lane < TRACK_MAXG) {
            const int g = lane;
            int cand = -1;
            if (gpresent_s[g] && map_s[g] >= 0)
                for (int j = 0; j < T && cand < 0; ++j)
                    if (hid_s[j] == map_s[g] && iou_s[g * TRACK_MAXT + j] > a.tau) cand = j;
            cand_s[g] = cand;
        }
        __syncthreads();
        if (lane == 0)
            for (int g = 0; g < G; ++g) {
                const int c = cand_s[g];
                if (c >= 0 && !jused_s[c]) {
                    gm_s[g] = c;
                    jused_s[c] = 1;
                }
            }
        __syncthreads();
        // ---- 2. the rest greedily by IoU ---------------------------------------------------------------------------------------------------
        for (;;) {
            double v = -1.0;
            int key = INT_MAX, pos = -1;
#pragma unroll
            for (int q = 0; q < TRACK_MAXG * TRACK_MAXT / 64; ++q) {
                const int p = lane + q * 64, g = p >> 5, j = p & 31;
                const double x = iou_s[p];
                if (gpresent_s[g] && gm_s[g] < 0 && hid_s[j] >= 0 && !jused_s[j] && x > a.tau) track_take_better(v, key, pos, x, p, p);
            }
            track_wave_argmax(v, key, pos);
            if (pos < 0) break;                                    // wave-uniform
            if (lane == 0) {
                gm_s[pos >> 5] = pos & 31;
                jused_s[pos & 31] = 1;
            }
            __syncthreads();
        }
        __syncthreads();
        // ---- 3., 4. switches and counters -----------------------------------------------------------------------------------------------------
        const int unmatched = __popcll(__ballot(lane < TRACK_MAXT && hid_s[lane & 31] >= 0 && !jused_s[lane & 31]));
        if (lane < G) a.gt_match[(size_t)r * G + lane] = gm_s[lane];
        if (lane == 0) {
            n_fp += unmatched;
            for (int g = 0; g < G; ++g) {
                if (!gpresent_s[g]) continue;
                ++n_gt;
                frames_s[g] += 1;
                const int j = gm_s[g];
                if (j < 0) {
                    ++n_miss;
                    continue;
                }
                ++n_match;
                tracked_s[g] += 1;
                sum_iou = sum_iou + iou_s[g * TRACK_MAXT + j];
                const int id = hid_s[j];
                n_idsw += (map_s[g] >= 0 && map_s[g] != id) ? 1 : 0;
                map_s[g] = id;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        int mt = 0, ml = 0, objects = 0;
        for (int g = 0; g < G; ++g) {
            if (frames_s[g] <= 0) continue;
            ++objects;
            mt += 5 * tracked_s[g] >= 4 * frames_s[g] ? 1 : 0;
            ml += 5 * tracked_s[g] <= frames_s[g] ? 1 : 0;
        }
        int *c = a.seq_counts + (size_t)s * 8;
        c[0] = n_gt, c[1] = n_match, c[2] = n_miss, c[3] = n_fp, c[4] = n_idsw, c[5] = mt, c[6] = ml, c[7] = objects;
        a.seq_iou[s] = sum_iou;
    }
    if constexpr (STREAM) {
        int *c = a.st_i + (size_t)s * TRACK_SCORE_ST;
        if (lane == 0) {
            c[0] = n_gt, c[1] = n_match, c[2] = n_miss, c[3] = n_fp, c[4] = n_idsw;
            a.st_f[s] = sum_iou;
        }
        if (lane < TRACK_MAXG) {
            c[8 + lane] = map_s[lane];
            c[16 + lane] = tracked_s[lane];
            c[24 + lane] = frames_s[lane];
        }
        for (int e = lane; e < (F - V) * G; e += 64) a.gt_match[((size_t)s * F + V) * G + e] = -1;      // the padding rows
    }
}

extern "C" int air_track_score(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, double tau,
                               int T, int G, int S, int F, int R, int *seq_counts, double *seq_iou, int *gt_match, void *stream) {
    AIR_REQUIRE(boxes && num_objects && track_id && gt_boxes && seq_counts && seq_iou && gt_match, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && G >= 1 && G <= TRACK_MAXG && S > 0 && F > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= TRACK_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(tau >= 0.0 && tau <= 1.0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(boxes) && air_aligned16(gt_boxes) && (reinterpret_cast<uintptr_t>(seq_iou) & 7u) == 0, AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(seq_counts) | reinterpret_cast<uintptr_t>(gt_match);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const TrackScoreArgs a = {boxes, gt_boxes, num_objects, track_id, seq_counts, gt_match, seq_iou, tau, T, G, S, F};
    hipLaunchKernelGGL(track_score_kernel<false>, dim3((unsigned)S), dim3(64), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

extern "C" int air_track_score_stream(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, double tau,
                                      int T, int G, int S, int F, int R, const int *valid, int *st_i, double *st_f, int *seq_counts,
                                      double *seq_iou, int *gt_match, void *stream) {
    AIR_REQUIRE(boxes && num_objects && track_id && gt_boxes && valid && st_i && st_f && seq_counts && seq_iou && gt_match, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && G >= 1 && G <= TRACK_MAXG && S > 0 && F > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= TRACK_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(tau >= 0.0 && tau <= 1.0, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(boxes) && air_aligned16(gt_boxes), AIR_E_ALIGN);
    AIR_REQUIRE(((reinterpret_cast<uintptr_t>(seq_iou) | reinterpret_cast<uintptr_t>(st_f)) & 7u) == 0, AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(valid) | reinterpret_cast<uintptr_t>(st_i) |
                           reinterpret_cast<uintptr_t>(seq_counts) | reinterpret_cast<uintptr_t>(gt_match);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    TrackScoreStreamArgs a;
    static_cast<TrackScoreArgs &>(a) = {boxes, gt_boxes, num_objects, track_id, seq_counts, gt_match, seq_iou, tau, T, G, S, F};
    a.valid = valid, a.st_i = st_i, a.st_f = st_f;
    hipLaunchKernelGGL(track_score_kernel<true>, dim3((unsigned)S), dim3(64), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// idf
// ============================================================================================================
struct TrackIdfArgs {
    const float *boxes, *gt_boxes;
    const int *num_objects, *track_id;
    int *overlap, *seq_idf;
    double tau;
    int T, G, S, F, n_ids;
};

// One 256-thread workgroup per sequence.  The frames: pair p = g * 32 + j, one per thread, then thread g alone adds to row g of the
// overlap table (no atomics: one writer per element).  The assignment: thread m holds best[m], the largest summed overlap of a
// one-to-one assignment of the ids visited so far to ground-truth slots within the subset m; 32 ids (256 table entries, one per
// thread) are staged per pass, an id without overlap is passed over.
__global__ __launch_bounds__(TRACK_THREADS) void track_idf_kernel(TrackIdfArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 hbox_s[TRACK_MAXT], gbox_s[TRACK_MAXG];
    __shared__ int hid_s[TRACK_MAXT], gpresent_s[TRACK_MAXG], hit_s[TRACK_MAXG * TRACK_MAXT];
    __shared__ int col_s[TRACK_MAXT * TRACK_MAXG];                 // [id within the pass][g]
    __shared__ int best_s[2][1 << TRACK_MAXG];
    __shared__ int max_id_s;
    const int T = a.T, G = a.G, F = a.F, R = a.S * F, n_ids = a.n_ids;
    const int s = blockIdx.x, tid = threadIdx.x;
    int *table = a.overlap + (size_t)s * G * n_ids;
    for (int e = tid; e < G * n_ids; e += TRACK_THREADS) table[e] = 0;
    if (tid == 0) max_id_s = -1;
    int gt_frames = 0, hyp_frames = 0, max_id = -1;                // thread 0's
    __syncthreads();
    for (int f = 0; f < F; ++f) {
        const int r = s * F + f;
        int n = a.num_objects[r];
        n = n < 0 ? 0 : (n > T ? T : n);
        if (tid < TRACK_MAXT) {
            const int j = tid;
            float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
            int id = -1;
            if (j < n) {
                const size_t row = (size_t)j * R + r;
                box = *reinterpret_cast<const float4 *>(a.boxes + 4 * row);
                const int t = a.track_id[row];
                if (t >= 0 && track_finite4(box)) id = t;
            }
            hbox_s[j] = box;
            hid_s[j] = id;
        }
        if (tid >= 64 && tid < 64 + TRACK_MAXG) {                  // (the second wavefront: the two loads go side by side)
            const int g = tid - 64;
            float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < G) gb = *reinterpret_cast<const float4 *>(a.gt_boxes + 4 * ((size_t)r * G + g));
            gbox_s[g] = gb;
            gpresent_s[g] = (g < G && gb.z > 0.f) ? 1 : 0;
        }
        __syncthreads();
        {
            const int g = tid >> 5, j = tid & 31, id = hid_s[j];
            hit_s[tid] = (gpresent_s[g] && id >= 0 && id < n_ids && box_iou_f64(gbox_s[g], hbox_s[j]) > a.tau) ? 1 : 0;
        }
        __syncthreads();
        if (tid < G && gpresent_s[tid])
            for (int j = 0; j < T; ++j)
                if (hit_s[tid * TRACK_MAXT + j]) table[(size_t)tid * n_ids + hid_s[j]] += 1;
        if (tid == 0) {
            for (int g = 0; g < G; ++g) gt_frames += gpresent_s[g];
            for (int j = 0; j < T; ++j) {
                const int id = hid_s[j];
                hyp_frames += id >= 0 ? 1 : 0;
                if (id < n_ids && id > max_id) max_id = id;
            }
        }
        __syncthreads();
    }
    if (tid == 0) max_id_s = max_id;
    best_s[0][tid] = 0;
    __syncthreads();                                               // the table is complete, and visible to the whole workgroup
    const int last_id = max_id_s, full = (1 << G) - 1;
    int cur = 0, with_overlap = 0;
    for (int id0 = 0; id0 <= last_id; id0 += TRACK_MAXT) {
        {
            const int g = tid >> 5, id = id0 + (tid & 31);
            col_s[(tid & 31) * TRACK_MAXG + g] = (g < G && id <= last_id) ? table[(size_t)g * n_ids + id] : 0;
        }
        __syncthreads();
        for (int q = 0; q < TRACK_MAXT && id0 + q <= last_id; ++q) {
            const int *col = col_s + q * TRACK_MAXG;
            int any = 0;
#pragma unroll
            for (int g = 0; g < TRACK_MAXG; ++g) any |= col[g];
            if (!any) continue;                                    // workgroup-uniform
            ++with_overlap;
            int b = best_s[cur][tid];
            if (tid <= full) {
#pragma unroll
                for (int g = 0; g < TRACK_MAXG; ++g)
                    if ((tid >> g) & 1) {
                        const int c = best_s[cur][tid ^ (1 << g)] + col[g];
                        b = c > b ? c : b;
                    }
            }
            best_s[cur ^ 1][tid] = b;
            cur ^= 1;
            __syncthreads();
        }
        __syncthreads();                                           // (col_s is restaged)
    }
    if (tid == 0) {
        int *o = a.seq_idf + (size_t)s * 4;
        o[0] = best_s[cur][full], o[1] = gt_frames, o[2] = hyp_frames, o[3] = with_overlap;
    }
}

extern "C" int air_track_idf(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, double tau, int T,
                             int G, int S, int F, int R, int n_ids, int *overlap, int *seq_idf, void *stream) {
    AIR_REQUIRE(boxes && num_objects && track_id && gt_boxes && overlap && seq_idf, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && G >= 1 && G <= TRACK_MAXG && S > 0 && F > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= TRACK_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(tau >= 0.0 && tau <= 1.0 && n_ids >= 1 && n_ids <= TRACK_MAX_IDS, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(boxes) && air_aligned16(gt_boxes), AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(overlap) | reinterpret_cast<uintptr_t>(seq_idf);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const TrackIdfArgs a = {boxes, gt_boxes, num_objects, track_id, overlap, seq_idf, tau, T, G, S, F, n_ids};
    hipLaunchKernelGGL(track_idf_kernel, dim3((unsigned)S), dim3(TRACK_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// hota
// ============================================================================================================
struct TrackHotaArgs {
    const float *boxes, *gt_boxes;
    const int *num_objects, *track_id;
    double *potential, *seq_hota_f;
    int *id_count, *gt_count, *matches, *seq_hota_i;
    int T, G, S, F, n_ids;
};
#define TRACK_HOTA_ALPHAS 19             // alpha_k = k / 20.0, k = 1..19

// One 256-thread workgroup per sequence; both passes over the frames run here.  The staging and the pair p = g * 32 + j, one per
// thread, are track_idf_kernel's; a hypothesis that takes part has 0 <= id < n_ids.  Pass 1: thread (g, j) adds to pot[g, id_j] when j
// is the first hypothesis of its id in the frame -- then it adds the frame's terms of that id in ascending j, so every element has one
// writer per frame and the order is the stated one; thread j likewise adds the frame's count of its id to ic.  Pass 2: the int64
// profits in LDS, wavefront 0 runs track_solve_wave (columns g < G, every other slot column forbidden), thread (a, g) books the match
// of slot g at threshold a, thread a adds tp and loc over g in ascending order.  The end: thread (a, g) adds the ids in ascending
// order, thread a the slots.  The tables are global memory written and read by this workgroup alone, a barrier between the two.
__global__ __launch_bounds__(TRACK_THREADS) void track_hota_kernel(TrackHotaArgs a) {
#pragma clang fp contract(off)
    __shared__ long long profit_s[TRACK_MAXT * TRACK_MAXT];        // [column k][object j]; columns >= 8 stay forbidden
    __shared__ double sim_s[TRACK_MAXG * TRACK_MAXT], rs_s[TRACK_MAXG], cs_s[TRACK_MAXT];
    __shared__ double part_s[3][TRACK_HOTA_ALPHAS * TRACK_MAXG];
    __shared__ float4 hbox_s[TRACK_MAXT], gbox_s[TRACK_MAXG];
    __shared__ int hid_s[TRACK_MAXT], hyp_s[TRACK_MAXT], ostate_s[TRACK_MAXT], gpresent_s[TRACK_MAXG], gc_s[TRACK_MAXG];
    __shared__ int match_s[TRACK_MAXG], max_id_s, dets_s[2];
    const int T = a.T, G = a.G, F = a.F, R = a.S * F, n_ids = a.n_ids;
    const int s = blockIdx.x, tid = threadIdx.x;
    double *pot = a.potential + (size_t)s * G * n_ids;
    int *ic = a.id_count + (size_t)s * n_ids;
    int *mat = a.matches + (size_t)s * TRACK_HOTA_ALPHAS * G * n_ids;
    for (int e = tid; e < G * n_ids; e += TRACK_THREADS) pot[e] = 0.0;
    for (int e = tid; e < n_ids; e += TRACK_THREADS) ic[e] = 0;
    for (int e = tid; e < TRACK_HOTA_ALPHAS * G * n_ids; e += TRACK_THREADS) mat[e] = 0;
    for (int e = tid; e < TRACK_MAXT * TRACK_MAXT; e += TRACK_THREADS) profit_s[e] = -1;
    if (tid < TRACK_MAXG) gc_s[tid] = 0;
    if (tid == 0) max_id_s = -1;
    int gt_dets = 0, hyp_dets = 0;                                 // thread 0's, thread 128's
    int tp = 0;                                                    // thread 192 + a: its threshold's
    double loc = 0.0;
    const int pg = tid >> 5, pj = tid & 31;                        // this thread's pair
    const int ba = tid >> 3, bg = tid & 7;                         // this thread's (threshold, slot), ba < 19
    const double alpha = (double)(ba + 1) / 20.0;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        for (int f = 0; f < F; ++f) {
            const int r = s * F + f;
            int n = a.num_objects[r];
            n = n < 0 ? 0 : (n > T ? T : n);
            if (tid < TRACK_MAXT) {
                const int j = tid;
                float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
                int id = -1, hyp = 0;
                if (j < n) {
                    const size_t row = (size_t)j * R + r;
                    box = *reinterpret_cast<const float4 *>(a.boxes + 4 * row);
                    const int t = a.track_id[row];
                    if (t >= 0 && track_finite4(box)) {
                        hyp = 1;
                        if (t < n_ids) id = t;
                    }
                }
                hbox_s[j] = box;
                hid_s[j] = id;                                     // -1: takes no part
                hyp_s[j] = hyp;
                ostate_s[j] = id >= 0 ? TRACK_UNCONFIRMED : TRACK_ABSENT;
            }
            if (tid >= 64 && tid < 64 + TRACK_MAXG) {
                const int g = tid - 64;
                float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g < G) gb = *reinterpret_cast<const float4 *>(a.gt_boxes + 4 * ((size_t)r * G + g));
                gbox_s[g] = gb;
                gpresent_s[g] = (g < G && gb.z > 0.f) ? 1 : 0;
                match_s[g] = -1;
            }
            __syncthreads();
            const int id = hid_s[pj];
            const double sim = (gpresent_s[pg] && id >= 0) ? box_iou_f64(gbox_s[pg], hbox_s[pj]) : 0.0;
            sim_s[tid] = sim;
            __syncthreads();
            if (pass == 0) {
                if (tid < TRACK_MAXG) {                            // rs[g]: ascending j (a pair that is none adds +0)
                    double v = 0.0;
                    for (int j = 0; j < TRACK_MAXT; ++j) v = v + sim_s[tid * TRACK_MAXT + j];
                    rs_s[tid] = v;
                    gc_s[tid] += gpresent_s[tid];
                }
                if (tid >= 64 && tid < 64 + TRACK_MAXT) {          // cs[j]: ascending g
                    const int j = tid - 64;
                    double v = 0.0;
                    for (int g = 0; g < TRACK_MAXG; ++g) v = v + sim_s[g * TRACK_MAXT + j];
                    cs_s[j] = v;
                }
                if (tid == 0)
                    for (int g = 0; g < TRACK_MAXG; ++g) gt_dets += gpresent_s[g];
                if (tid == 128) {
                    int h = 0, top = max_id_s;
                    for (int j = 0; j < TRACK_MAXT; ++j) {
                        h += hyp_s[j];
                        top = hid_s[j] > top ? hid_s[j] : top;
                    }
                    hyp_dets += h;
                    max_id_s = top;
                }
                __syncthreads();
                if (id >= 0) {
                    bool first = true;
                    for (int j = 0; j < pj; ++j) first = first && hid_s[j] != id;
                    if (first) {
                        if (gpresent_s[pg]) {
                            double v = pot[(size_t)pg * n_ids + id];
                            const double rsg = rs_s[pg];
                            for (int j = pj; j < TRACK_MAXT; ++j) {
                                if (hid_s[j] != id) continue;
                                const double sj = sim_s[pg * TRACK_MAXT + j];
                                const double d = (cs_s[j] + rsg) - sj;
                                if (d > 0x1p-52) v = v + sj / d;
                            }
                            pot[(size_t)pg * n_ids + id] = v;
                        }
                        if (pg == 0) {
                            int c = 0;
                            for (int j = pj; j < TRACK_MAXT; ++j) c += hid_s[j] == id ? 1 : 0;
                            ic[id] += c;
                        }
                    }
                }
            } else {
                if (sim > 0.0) {                                   // admissible: present g < G, 0 <= id < n_ids
                    const double p = pot[(size_t)pg * n_ids + id];
                    const double A = p / (((double)gc_s[pg] + (double)ic[id]) - p);
                    profit_s[tid] = 1 + (long long)floor((A * sim) * 4294967296.0);
                } else {
                    profit_s[tid] = -1;
                }
                __syncthreads();
                if (tid < 64) {                                    // wavefront 0, every lane
                    const int row = track_solve_wave(profit_s, ostate_s, T, tid);
                    if (tid < G) match_s[tid] = row;
                }
                __syncthreads();
                if (ba < TRACK_HOTA_ALPHAS && bg < G) {
                    const int j = match_s[bg];
                    if (j >= 0 && sim_s[bg * TRACK_MAXT + j] >= alpha) mat[((size_t)ba * G + bg) * n_ids + hid_s[j]] += 1;
                }
                if (tid >= 192 && tid < 192 + TRACK_HOTA_ALPHAS) { // thread a: the matched pairs in ascending g
                    const double al = (double)(tid - 192 + 1) / 20.0;
                    for (int g = 0; g < G; ++g) {
                        const int j = match_s[g];
                        if (j < 0) continue;
                        const double sj = sim_s[g * TRACK_MAXT + j];
                        if (sj >= al) {
                            tp += 1;
                            loc = loc + sj;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) dets_s[0] = gt_dets;
    if (tid == 128) dets_s[1] = hyp_dets;
    __syncthreads();
    const int last_id = max_id_s;
    if (ba < TRACK_HOTA_ALPHAS) {
        double ass = 0.0, ass_re = 0.0, ass_pr = 0.0;
        if (bg < G) {
            const int *m = mat + ((size_t)ba * G + bg) * n_ids;
            const double gcg = (double)gc_s[bg];
            for (int i = 0; i <= last_id; ++i) {
                const int ci = m[i];
                if (ci <= 0) continue;
                const double c = (double)ci, ici = (double)ic[i];
                ass = ass + c * (c / ((gcg + ici) - c));
                ass_re = ass_re + c * (c / gcg);
                ass_pr = ass_pr + c * (c / ici);
            }
        }
        part_s[0][tid] = ass, part_s[1][tid] = ass_re, part_s[2][tid] = ass_pr;
    }
    __syncthreads();
    if (tid < TRACK_MAXG && tid < G) a.gt_count[(size_t)s * G + tid] = gc_s[tid];
    if (tid >= 192 && tid < 192 + TRACK_HOTA_ALPHAS) {
        const int k = tid - 192;
        double v[3] = {0.0, 0.0, 0.0};
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = v[q] + part_s[q][k * TRACK_MAXG + g];
        int *oi = a.seq_hota_i + ((size_t)s * TRACK_HOTA_ALPHAS + k) * 3;
        double *of = a.seq_hota_f + ((size_t)s * TRACK_HOTA_ALPHAS + k) * 4;
        oi[0] = tp, oi[1] = dets_s[0] - tp, oi[2] = dets_s[1] - tp;
        of[0] = v[0], of[1] = v[1], of[2] = v[2], of[3] = loc;
    }
}

extern "C" int air_track_hota(const float *boxes, const int *num_objects, const int *track_id, const float *gt_boxes, int T, int G,
                              int S, int F, int R, int n_ids, double *potential, int *id_count, int *gt_count, int *matches,
                              int *seq_hota_i, double *seq_hota_f, void *stream) {
    AIR_REQUIRE(boxes && num_objects && track_id && gt_boxes && potential && id_count && gt_count && matches && seq_hota_i &&
                    seq_hota_f, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && G >= 1 && G <= TRACK_MAXG && S > 0 && F > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= TRACK_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(n_ids >= 1 && n_ids <= TRACK_MAX_IDS, AIR_E_SHAPE);
    AIR_REQUIRE((long)S * TRACK_HOTA_ALPHAS * G * n_ids <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(boxes) && air_aligned16(gt_boxes), AIR_E_ALIGN);
    AIR_REQUIRE(((reinterpret_cast<uintptr_t>(potential) | reinterpret_cast<uintptr_t>(seq_hota_f)) & 7u) == 0, AIR_E_ALIGN);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(num_objects) | reinterpret_cast<uintptr_t>(track_id) |
                           reinterpret_cast<uintptr_t>(id_count) | reinterpret_cast<uintptr_t>(gt_count) |
                           reinterpret_cast<uintptr_t>(matches) | reinterpret_cast<uintptr_t>(seq_hota_i);
    AIR_REQUIRE((bits & 3u) == 0, AIR_E_ALIGN);
    const TrackHotaArgs a = {boxes, gt_boxes, num_objects, track_id, potential, seq_hota_f, id_count, gt_count, matches, seq_hota_i,
                             T, G, S, F, n_ids};
    hipLaunchKernelGGL(track_hota_kernel, dim3((unsigned)S), dim3(TRACK_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// mots
// ============================================================================================================
struct TrackMotsArgs {
    const int *cont, *num_objects, *track_id;
    int *seq_mots_i, *mots_match;
    double *seq_mots_f;
    float *mots_iou;
    int T, G, S, F;
};
#define TRACK_MOTS_BINS ((TRACK_MAXT + 1) * (TRACK_MAXG + 1))      // 297 counts per frame at most
#define TRACK_MOTS_LOADS ((TRACK_MOTS_BINS + 63) / 64)             // 5 per lane

// what one lane holds of a frame between its loads and its turn: its share of the counts, the frame's count, step `lane`'s id
struct TrackMotsFrame {
    int c[TRACK_MOTS_LOADS];
    int n, id;
};
__device__ __forceinline__ void track_mots_load(TrackMotsFrame &x, const TrackMotsArgs &a, int r, int R, int nb, int lane) {
    const int *c = a.cont + (size_t)r * nb;
#pragma unroll
    for (int k = 0; k < TRACK_MOTS_LOADS; ++k) {
        const int i = lane + 64 * k;
        x.c[k] = i < nb ? c[i] : 0;
    }
    x.n = a.num_objects[r];
    x.id = lane < a.T ? a.track_id[(size_t)lane * R + r] : -1;
}

// One workgroup of one wavefront per sequence, the frames walked in order.  A frame's (T+1)(G+1) counts go global -> registers -> LDS;
// the loads of frame f + 1 are issued behind the barrier that publishes frame f, so they are in flight while f is booked.  Lane =
// step j for the row sums and the match test (one ballot per slot), lane = slot g for map, tracked and present, which never leave
// their lane's registers.  inter > union - inter decides in int64.  For a non-negative table at most one step qualifies per slot
// and at most one slot per step (a match holds more than half of both areas), so taking the LOWEST qualifying step of a slot, as
// the ballot does, is no tie rule: any search order gives the same matching.
__global__ __launch_bounds__(64) void track_mots_kernel(TrackMotsArgs a) {
#pragma clang fp contract(off)
    __shared__ int cont_s[TRACK_MOTS_BINS];
    __shared__ long long row_s[TRACK_MAXT];
    __shared__ long long col_s[TRACK_MAXG];
    __shared__ int id_s[TRACK_MAXT];
    const int T = a.T, G = a.G, F = a.F, R = a.S * F, W = G + 1, nb = (T + 1) * W;
    const int s = blockIdx.x, lane = threadIdx.x;
    int map = -1, tracked = 0, frames = 0, switches = 0;           // lane g's
    int n_gt = 0, n_tp = 0, n_fn = 0, n_fp = 0;                    // wave-uniform
    double soft = 0.0;                                             // wave-uniform
    TrackMotsFrame next;
    track_mots_load(next, a, s * F, R, nb, lane);
    for (int f = 0; f < F; ++f) {
        const int r = s * F + f;
#pragma unroll
        for (int k = 0; k < TRACK_MOTS_LOADS; ++k) {
            const int i = lane + 64 * k;
            if (i < nb) cont_s[i] = next.c[k];
        }
        const int n = next.n < 0 ? 0 : (next.n > T ? T : next.n), id = next.id;
        __syncthreads();
        if (f + 1 < F) track_mots_load(next, a, r + 1, R, nb, lane);
        long long row = 0, col = 0;
        if (lane < T)
            for (int b = 0; b < W; ++b) row += (long long)cont_s[(lane + 1) * W + b];
        if (lane < G)
            for (int o = 0; o <= T; ++o) col += (long long)cont_s[o * W + lane + 1];
        const bool hyp = lane < n && id >= 0 && row > 0;
        if (lane < TRACK_MAXT) {
            row_s[lane] = row;
            id_s[lane] = id;
        }
        if (lane < TRACK_MAXG) col_s[lane] = col;
        __syncthreads();
        // ---- the match test: lane j against every present slot -----------------------------------------------------------------------------
        bool taken = false;
        int mine = -1;                                             // lane g: the step matched to slot g
#pragma unroll
        for (int g = 0; g < TRACK_MAXG; ++g) {
            bool q = false;
            if (g < G && hyp) {
                const long long cg = col_s[g];
                if (cg > 0) {
                    const long long inter = (long long)cont_s[(lane + 1) * W + g + 1], uni = row + cg - inter;
                    q = inter > uni - inter;
                }
            }
            const unsigned long long m = __ballot(q);
            const int j = m ? __ffsll(m) - 1 : -1;
            taken = taken || (q && lane == j);
            if (lane == g) mine = j;
        }
        // ---- booking: lane g ---------------------------------------------------------------------------------------------------------------
        const bool here = lane < G && col > 0, hit = here && mine >= 0;
        double iou = 0.0;
        if (hit) {
            const long long inter = (long long)cont_s[(mine + 1) * W + lane + 1], uni = row_s[mine] + col - inter;
            iou = (double)inter / (double)uni;
            const int idj = id_s[mine];
            switches += (map >= 0 && map != idj) ? 1 : 0;
            map = idj;
            tracked += 1;
        }
        frames += here ? 1 : 0;
        if (lane < G) {
            a.mots_match[(size_t)r * G + lane] = hit ? mine : -1;
            a.mots_iou[(size_t)r * G + lane] = (float)iou;
        }
#pragma unroll
        for (int g = 0; g < TRACK_MAXG; ++g) soft = soft + __shfl(iou, g, 64);      // g order; an unmatched slot adds +0: no change of bits
        const int hits = __popcll(__ballot(hit)), there = __popcll(__ballot(here));
        n_gt += there;
        n_tp += hits;
        n_fn += there - hits;
        n_fp += __popcll(__ballot(hyp && !taken));
        __syncthreads();                                           // the next frame overwrites the counts
    }
    const bool object = lane < G && frames > 0;
    const int objects = __popcll(__ballot(object));
    const int mt = __popcll(__ballot(object && 5ll * tracked >= 4ll * frames));
    const int ml = __popcll(__ballot(object && 5ll * tracked <= (long long)frames));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) switches += __shfl_xor(switches, off, 64);
    if (lane == 0) {
        int *c = a.seq_mots_i + (size_t)s * 8;
        c[0] = n_gt, c[1] = n_tp, c[2] = n_fn, c[3] = n_fp, c[4] = switches, c[5] = mt, c[6] = ml, c[7] = objects;
        a.seq_mots_f[s] = soft;
    }
}

extern "C" int air_track_mots(const int *cont, const int *num_objects, const int *track_id, int T, int G, int S, int F, int R,
                              int *seq_mots_i, double *seq_mots_f, int *mots_match, float *mots_iou, void *stream) {
    AIR_REQUIRE(cont && num_objects && track_id && seq_mots_i && seq_mots_f && mots_match && mots_iou, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && G >= 1 && G <= TRACK_MAXG && S > 0 && F > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)S * F == (long)R && (long)R * (T + 1) * (G + 1) <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE((reinterpret_cast<uintptr_t>(seq_mots_f) & 7u) == 0, AIR_E_ALIGN);
    AIR_REQUIRE(track_aligned4({cont, num_objects, track_id, seq_mots_i, mots_match, mots_iou}), AIR_E_ALIGN);
    const TrackMotsArgs a = {cont, num_objects, track_id, seq_mots_i, mots_match, seq_mots_f, mots_iou, T, G, S, F};
    hipLaunchKernelGGL(track_mots_kernel, dim3((unsigned)S), dim3(64), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}

// ============================================================================================================
// stitch
// ============================================================================================================
struct TrackStitchArgs {
    const float *what, *where;
    const int *track_id, *num_tracks, *track_first, *track_last, *track_length, *track_gaps;
    int *stitch_id, *stitch_parent, *stitch_root, *stitch_first, *stitch_last, *stitch_length, *stitch_gaps, *num_links, *stitch_status;
    float *stitch_d2, *stitch_affinity;
    double gate_d2, w, q[2], r, velocity_var;      // q[0]: the shifts, q[1]: the scales (TrackMotionArgs')
    int T, S, F, A, max_gap;
};

// One 256-thread workgroup per sequence; N = the ids issued, at most 32 (more: the sequence is copied through, status 1).
//   filter   lane i < N of wavefront 0 walks the frames clip(first[i]) .. clip(last[i]) of its id one by one -- the slot of a sighting is
//            the lowest j with track_id == i -- and runs the tracker's own filter statements: a start at the first sighting; at a later
//            one, m frames on, m - 1 predicts one by one, then a predict and TRAJ_UPDATE.  It keeps the 14 doubles in registers and the
//            (frame, slot) of its first and last sighting and the first sighting's `where` row in LDS.
//   predict  the same lane then predicts on, one frame at a time, up to max_gap frames or the end of the sequence; at step g it
//            writes its predicted state into its own column of gstate_s and scores, by track_gate_d2, every b whose first sighting
//            is frame last + g: one d2 per candidate pair, no loop over the gap per pair.  d2_s[a * 32 + b], -1 for no candidate.
//   pairs    pair p = a * 32 + b, four per thread: the association's msd loop over the `what` rows of a's last and b's first sighting,
//            aff and the int64 profit, laid out as track_solve_wave reads them (column a, row b).
//   links    wavefront 0 runs track_solve_wave, unchanged: lane a < 32 gets the row b linked behind track a.
//   relabel  lane i follows parent to its root and, if it is a root, the children to the tail; every thread relabels stitch_id and
//            copies the table rows from N on.
// Float64 with contraction off, one writer per output element, no atomics.
__global__ __launch_bounds__(TRACK_THREADS) void track_stitch_kernel(TrackStitchArgs a) {
#pragma clang fp contract(off)
    __shared__ double gstate_s[TRACK_GS_DOUBLES * TRACK_MAXT];     // the predicted state of track a at the current step: its own column
    __shared__ double d2_s[TRACK_MAXT * TRACK_MAXT], aff_s[TRACK_MAXT * TRACK_MAXT];
    __shared__ long long profit_s[TRACK_MAXT * TRACK_MAXT];        // [column a][row b]
    __shared__ float4 fwhere_s[TRACK_MAXT];                        // the `where` row of the first sighting
    __shared__ int ff_s[TRACK_MAXT], fj_s[TRACK_MAXT], lf_s[TRACK_MAXT], lj_s[TRACK_MAXT];      // first / last sighting: frame (-1: none), slot
    __shared__ int ostate_s[TRACK_MAXT], parent_s[TRACK_MAXT], child_s[TRACK_MAXT], root_s[TRACK_MAXT];
    const int T = a.T, F = a.F, A = a.A, R = a.S * F, FT = F * T;
    const int s = blockIdx.x, tid = threadIdx.x;
    const size_t tab = (size_t)s * FT;
    int N = a.num_tracks[s];
    N = N < 0 ? 0 : N;
    if (N <= TRACK_MAXT && N > FT) N = FT;                         // (no more ids than objects: the table rows end at F T)
    if (N > TRACK_MAXT) {                                         // OVERFLOW (workgroup-uniform): bit copies, no link
        for (int e = tid; e < FT; e += TRACK_THREADS) {
            const int f = e / T, j = e - f * T;
            const size_t row = (size_t)j * R + (size_t)s * F + f;
            a.stitch_id[row] = a.track_id[row];
            a.stitch_first[tab + e] = a.track_first[tab + e];
            a.stitch_last[tab + e] = a.track_last[tab + e];
            a.stitch_length[tab + e] = a.track_length[tab + e];
            a.stitch_gaps[tab + e] = a.track_gaps[tab + e];
        }
        if (tid < TRACK_MAXT) {
            const size_t at = (size_t)s * TRACK_MAXT + tid;
            a.stitch_parent[at] = -1;
            a.stitch_root[at] = tid;
            a.stitch_d2[at] = 0.f;
            a.stitch_affinity[at] = 0.f;
        }
        if (tid == 0) {
            a.num_links[s] = 0;
            a.stitch_status[s] = 1;
        }
        return;
    }
    for (int p = tid; p < TRACK_MAXT * TRACK_MAXT; p += TRACK_THREADS) d2_s[p] = -1.0;
    // ---- filter: lane i = id i -----------------------------------------------------------------------------------------------------------
    double x[4], v[4];
    TrajCov P[2];
    int lastf = -1;                                                // the frame of this lane's last sighting
    const double q2[2] = {0.5 * a.q[0], 0.5 * a.q[1]}, q4[2] = {0.25 * a.q[0], 0.25 * a.q[1]};
    if (tid < TRACK_MAXT) {
        const int i = tid;
        int ff = -1, fj = -1, lj = -1;
        float4 fw = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = 0.0, v[c] = 0.0;
        P[0].xx = P[1].xx = P[0].xv = P[1].xv = P[0].vv = P[1].vv = 0.0;
        if (i < N) {
            int f0 = a.track_first[tab + i], f1 = a.track_last[tab + i];
            f0 = f0 < 0 ? 0 : (f0 > F - 1 ? F - 1 : f0);
            f1 = f1 < 0 ? 0 : (f1 > F - 1 ? F - 1 : f1);
            for (int f = f0; f <= f1; ++f) {
                const size_t r = (size_t)s * F + f;
                int j = 0;
                while (j < T && a.track_id[(size_t)j * R + r] != i) ++j;
                if (j == T) continue;                              // not sighted in this frame: predicted when the next sighting is booked
                const float4 w4 = *reinterpret_cast<const float4 *>(a.where + 4 * ((size_t)j * R + r));
                if (ff < 0) {                                      // start: x = z, v = 0, P = (r, 0, velocity_var)
                    fw = w4;
                    x[0] = (double)w4.x, x[1] = (double)w4.y, x[2] = (double)w4.z, x[3] = (double)w4.w;
                    P[0].xx = P[1].xx = a.r;
                    P[0].vv = P[1].vv = a.velocity_var;
                    ff = f, fj = j;
                } else {                                           // the frames coasted over one by one, then the update
                    const double z[4] = {(double)w4.x, (double)w4.y, (double)w4.z, (double)w4.w};
                    const int m = f - lastf;
                    for (int i2 = 1; i2 < m; ++i2) {
#pragma unroll
                        for (int c = 0; c < 2; ++c) P[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) x[c] = x[c] + v[c];
                    }
                    TrajCov Pp[2];
                    double xp[4], vp[4];
#pragma unroll
                    for (int c = 0; c < 2; ++c) Pp[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) xp[c] = x[c] + v[c], vp[c] = v[c];
                    TRAJ_UPDATE(P, Pp, x, v, xp, vp, z, a.r)
                }
                lastf = f, lj = j;
            }
        }
        ff_s[i] = ff, fj_s[i] = fj, lf_s[i] = lastf, lj_s[i] = lj;
        fwhere_s[i] = fw;
        ostate_s[i] = i < N ? TRACK_UNCONFIRMED : TRACK_ABSENT;
        parent_s[i] = -1;
    }
    __syncthreads();
    // ---- predict: lane a one frame at a time; at step g the b that begin in frame last + g -------------------------------------------------
    if (tid < N && lastf >= 0) {                                   // (x, v, P: the filtered state at the last sighting)
        const int k = tid;
        int steps = F - 1 - lastf;
        steps = steps > a.max_gap ? a.max_gap : steps;
        double *gs = gstate_s + k;
        for (int g = 1; g <= steps; ++g) {
#pragma unroll
            for (int c = 0; c < 2; ++c) P[c] = traj_predict_cov(P[c], a.q[c], q2[c], q4[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = x[c] + v[c];
            bool staged = false;
            for (int b = 0; b < N; ++b) {
                if (ff_s[b] != lastf + g) continue;
                if (!staged) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) gs[(TRACK_GS_X + c) * TRACK_MAXT] = x[c];
#pragma unroll
                    for (int c = 0; c < 2; ++c) gs[(TRACK_GS_S + c) * TRACK_MAXT] = P[c].xx + a.r;
                    staged = true;
                }
                const double d2 = track_gate_d2(gstate_s, k, fwhere_s[b]);
                d2_s[k * TRACK_MAXT + b] = d2 <= a.gate_d2 ? d2 : -1.0;      // (a NaN or an inf fails the gate)
            }
        }
    }
    __syncthreads();
    // ---- pairs: msd, aff, profit -----------------------------------------------------------------------------------------------------------
    for (int p = tid; p < TRACK_MAXT * TRACK_MAXT; p += TRACK_THREADS) {
        const int k = p >> 5, b = p & 31;
        const double d2 = d2_s[p];
        double val = -1.0;
        if (d2 >= 0.0) {
            const float *wk = a.what + ((size_t)lj_s[k] * R + (size_t)s * F + lf_s[k]) * A;
            const float *wj = a.what + ((size_t)fj_s[b] * R + (size_t)s * F + ff_s[b]) * A;
            double sum = 0.0;
            int q = 0;
            for (; q + 8 <= A; q += 8) {                           // eight loads of each row in flight, added in ascending index
                float xs[8], ys[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    xs[u] = wk[q + u];
                    ys[u] = wj[q + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double d = (double)xs[u] - (double)ys[u];
                    sum = sum + d * d;
                }
            }
            for (; q < A; ++q) {
                const double d = (double)wk[q] - (double)wj[q];
                sum = sum + d * d;
            }
            const double msd = sum / (double)A;
            val = (1.0 - a.w) / (1.0 + d2) + a.w / (1.0 + msd);
        }
        const bool ok = val >= 0.0;                                // (a NaN aff takes no part)
        aff_s[p] = val;
        profit_s[p] = ok ? 1 + (long long)floor(val * 4294967296.0) : -1;      // (exact: a power of two)
    }
    __syncthreads();
    // ---- links -------------------------------------------------------------------------------------------------------------------------------
    if (tid < 64) {                                                // wavefront 0, every lane
        const int b = track_solve_wave(profit_s, ostate_s, N, tid);
        const bool linked = tid < TRACK_MAXT && b >= 0;
        const unsigned long long links = __ballot(linked);
        if (tid < TRACK_MAXT) child_s[tid] = linked ? b : -1;
        if (linked) parent_s[b] = tid;                             // one column per row: one writer
        if (tid == 0) {
            a.num_links[s] = __popcll(links);
            a.stitch_status[s] = 0;
        }
    }
    __syncthreads();
    // ---- relabel -----------------------------------------------------------------------------------------------------------------------------
    if (tid < TRACK_MAXT) {
        const int i = tid;
        const size_t at = (size_t)s * TRACK_MAXT + i;
        const int pa = parent_s[i];
        int root = -1;
        if (i < N) {
            root = i;
            for (int hop = 0; hop < TRACK_MAXT && parent_s[root] >= 0; ++hop) root = parent_s[root];
        }
        root_s[i] = root;
        a.stitch_parent[at] = pa;
        a.stitch_root[at] = root;
        a.stitch_d2[at] = pa >= 0 ? (float)d2_s[pa * TRACK_MAXT + i] : 0.f;
        a.stitch_affinity[at] = pa >= 0 ? (float)aff_s[pa * TRACK_MAXT + i] : 0.f;
        if (i < N) {
            int first = -1, last = -1, length = 0, gaps = 0;
            if (pa < 0) {                                          // a root: down the chain to its tail
                int c = i, links = 0;
                first = a.track_first[tab + i];
                for (int hop = 0; hop < TRACK_MAXT; ++hop) {
                    length += a.track_length[tab + c];
                    gaps += a.track_gaps[tab + c];
                    last = a.track_last[tab + c];
                    if (child_s[c] < 0) break;
                    c = child_s[c];
                    ++links;
                }
                gaps += links;
            }
            a.stitch_first[tab + i] = first;
            a.stitch_last[tab + i] = last;
            a.stitch_length[tab + i] = length;
            a.stitch_gaps[tab + i] = gaps;
        }
    }
    __syncthreads();
    for (int e = N + tid; e < FT; e += TRACK_THREADS) {            // the rows from N on: copied
        a.stitch_first[tab + e] = a.track_first[tab + e];
        a.stitch_last[tab + e] = a.track_last[tab + e];
        a.stitch_length[tab + e] = a.track_length[tab + e];
        a.stitch_gaps[tab + e] = a.track_gaps[tab + e];
    }
    for (int e = tid; e < FT; e += TRACK_THREADS) {
        const int f = e / T, j = e - f * T;
        const size_t row = (size_t)j * R + (size_t)s * F + f;
        const int id = a.track_id[row];
        a.stitch_id[row] = (id >= 0 && id < N) ? root_s[id] : id;
    }
}

extern "C" int air_track_stitch(const float *what, const float *where, const int *track_id, const int *num_tracks, const int *track_first,
                                const int *track_last, const int *track_length, const int *track_gaps, int T, int S, int F, int R,
                                int A, int max_gap, double gate_d2, double appearance_weight, double q_shift, double q_scale,
                                double measurement_noise, double velocity_var, int *stitch_id, int *stitch_parent, int *stitch_root,
                                float *stitch_d2, float *stitch_affinity, int *stitch_first, int *stitch_last, int *stitch_length,
                                int *stitch_gaps, int *num_links, int *stitch_status, void *stream) {
    AIR_REQUIRE(what && where && track_id && num_tracks && track_first && track_last && track_length && track_gaps && stitch_id &&
                    stitch_parent && stitch_root && stitch_d2 && stitch_affinity && stitch_first && stitch_last && stitch_length &&
                    stitch_gaps && num_links && stitch_status, AIR_E_NULL);
    AIR_REQUIRE(T >= 1 && T <= TRACK_MAXT && S > 0 && F > 0 && A > 0, AIR_E_SHAPE);
    AIR_REQUIRE((long)F * T <= TRACK_MAX_IDS && (long)S * F == (long)R && (long)S * F * T <= (long)INT_MAX, AIR_E_SHAPE);
    AIR_REQUIRE(max_gap >= 1 && isfinite(gate_d2) && gate_d2 > 0.0, AIR_E_SHAPE);
    AIR_REQUIRE(appearance_weight >= 0.0 && appearance_weight <= 1.0, AIR_E_SHAPE);
    AIR_REQUIRE(traj_noise_check(q_shift, q_scale, measurement_noise, velocity_var) == AIR_OK, AIR_E_SHAPE);
    AIR_REQUIRE(air_aligned16(where), AIR_E_ALIGN);
    AIR_REQUIRE(track_aligned4({what, track_id, num_tracks, track_first, track_last, track_length, track_gaps, stitch_id, stitch_parent,
                                stitch_root, stitch_d2, stitch_affinity, stitch_first, stitch_last, stitch_length, stitch_gaps, num_links,
                                stitch_status}), AIR_E_ALIGN);
    TrackStitchArgs a = {what, where, track_id, num_tracks, track_first, track_last, track_length, track_gaps, stitch_id, stitch_parent,
                         stitch_root, stitch_first, stitch_last, stitch_length, stitch_gaps, num_links, stitch_status, stitch_d2,
                         stitch_affinity, gate_d2, appearance_weight, {q_shift, q_scale}, measurement_noise, velocity_var, T, S, F, A,
                         max_gap};
    hipLaunchKernelGGL(track_stitch_kernel, dim3((unsigned)S), dim3(TRACK_THREADS), 0, air_stream(stream), a);
    AIR_LAUNCH_CHECK();
    return AIR_OK;
}
