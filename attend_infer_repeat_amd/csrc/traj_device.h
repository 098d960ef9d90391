// The constant-rate Kalman filter of the trajectory entries (include/air_hip.h states the rule), shared by the kernels that run it:
// air_track_smooth / air_track_smooth_stream (trajectory_kernels.hip) and the motion state of air_track_associate_motion
// (track_kernels.hip).  One text, so the filter inside the tracker and the smoother behind it are one filter, bit for bit.
#pragma once
#include "air_common.h"

struct TrajCov {
    double xx, xv, vv;
};

// predict: a = Pxx + Pxv, b = Pxv + Pvv, Pxx- = (a + b) + q4, Pxv- = b + q2, Pvv- = Pvv + q
__device__ __forceinline__ TrajCov traj_predict_cov(const TrajCov p, double q, double q2, double q4) {
#pragma clang fp contract(off)
    const double a = p.xx + p.xv, b = p.xv + p.vv;
    TrajCov o;
    o.xx = (a + b) + q4;
    o.xv = b + q2;
    o.vv = p.vv + q;
    return o;
}

// The update, shared by track_smooth_kernel, the stream kernels and the tracker's motion state as TEXT (the statements are those the
// one-shot kernel has always had, so its code object does not change with the sharing; a function would be inlined into another
// register allocation).  It is used under `#pragma clang fp contract(off)`.
// update with the sighting z:  s = Pxx- + r, kx = Pxx- / s, kv = Pxv- / s, P = P- - k P-;  e = z - x-, x = x- + kx e, v = v- + kv e
#define TRAJ_UPDATE(P, Pp, x, v, xp, vp, z, r_)                                                                               \
    {                                                                                                                         \
        double kx[2], kv[2];                                                                                                  \
        _Pragma("unroll") for (int c = 0; c < 2; ++c) {                                                                       \
            const double sn = Pp[c].xx + r_;                                                                                  \
            kx[c] = Pp[c].xx / sn;                                                                                            \
            kv[c] = Pp[c].xv / sn;                                                                                            \
            P[c].xx = Pp[c].xx - kx[c] * Pp[c].xx;                                                                            \
            P[c].xv = Pp[c].xv - kx[c] * Pp[c].xv;                                                                            \
            P[c].vv = Pp[c].vv - kv[c] * Pp[c].xv;                                                                            \
        }                                                                                                                     \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                                       \
            const int cl = (c & 1) ? 0 : 1; /* [sx, tx, sy, ty]: the odd components are shifts */                             \
            const double e = z[c] - xp[c];                                                                                    \
            x[c] = xp[c] + kx[cl] * e;                                                                                        \
            v[c] = vp[c] + kv[cl] * e;                                                                                        \
        }                                                                                                                     \
    }
// the rule's noise terms inside the supported domain (AIR_OK) or AIR_E_SHAPE: trajectory_kernels.hip defines it next to the domain
__attribute__((visibility("hidden"))) int traj_noise_check(double q_shift, double q_scale, double r, double velocity_var);
