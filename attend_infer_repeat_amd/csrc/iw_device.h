// What the importance-weight read-out (iw_kernels.hip) and its backward (iw_train_kernels.hip) share: the prior block, the step
// limit and the per-element log-ratio.
#pragma once
#include <math.h>
#include "scene_device.h"

#define IW_MAXT 32

struct IwPriors {
    float what_loc, what_scale, scale_loc, scale_scale, shift_loc, shift_scale;   // shift_loc NaN: centred on where_loc
};

// log N(x | p_loc, p_scale) - log N(x | loc, scale); the -1/2 log 2 pi terms cancel.  No clamps: a zero scale gives the
// +-inf / NaN of the plain formula.
__device__ __forceinline__ float iw_log_ratio(float x, float loc, float scale, float p_loc, float p_scale, float log_p_scale) {
    const float zq = (x - loc) / scale, zp = (x - p_loc) / p_scale;
    return 0.5f * (zq * zq - zp * zp) + (logf(scale) - log_p_scale);
}
