// The rigid change of frame of one box row (cmt_track_predict's pose, cmt_box_concat's transform): m is the 12
// floats of [R|t], row-major.  Every product and sum is rounded on its own, whatever the including file's flags:
// a position row is ((m0 x + m1 y) + m2 z) + t, the velocity goes through the upper-left 2 x 2.  The yaw stays
// with the callers: the tracker wraps it into [-pi, pi), the concat does not.
#pragma once
#include "cmt_common.h"

__device__ __forceinline__ void box_rigid(const float* m, float x, float y, float z, float vx, float vy, float (&pos)[3],
                                          float (&vel)[2]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float m0 = m[4 * a] * x, m1 = m[4 * a + 1] * y, m2 = m[4 * a + 2] * z;
        const float s01 = m0 + m1;
        const float s012 = s01 + m2;
        pos[a] = s012 + m[4 * a + 3];
    }
    const float a0 = m[0] * vx, a1 = m[1] * vy, b0 = m[4] * vx, b1 = m[5] * vy;
    vel[0] = a0 + a1;
    vel[1] = b0 + b1;
}
