// The inside test of include/cmt_hip.h (points_in_rbbox, the open interior) and the tile constants that
// ptsaug.hip and gtdb.hip share: both files stage a box and test a point with these instructions, so a point near
// a face falls on the same side in cmt_points_in_boxes, cmt_pts_augment and cmt_gtdb_extract.  Contraction is off
// in the row functions (and for both files, see the Makefile).
#pragma once
#include "wave_ops.h"

#include <cmath>

constexpr int AUG_T = TILE_T;         // slots (points) per tile
constexpr int AUG_THREADS = TILE_THREADS;
constexpr int AUG_R = AUG_T / AUG_THREADS;
constexpr int AUG_CHUNKS = AUG_T / 64;
constexpr int PIB_CB = 64;            // boxes staged per pass of cmt_points_in_boxes and cmt_gtdb_extract

struct aug_box {
    float cx, cy, zb, hx, hy, dz, c, s;
};

__device__ __forceinline__ aug_box aug_stage(const float* b) {
#pragma clang fp contract(off)
    aug_box o;
    o.cx = b[0], o.cy = b[1], o.zb = b[2];
    o.hx = b[3] * 0.5f, o.hy = b[4] * 0.5f, o.dz = b[5];
    o.c = cosf(b[6]), o.s = sinf(b[6]);
    return o;
}

// every comparison is false for a NaN operand: a NaN in the point or the box gives "outside"
__device__ __forceinline__ bool aug_inside(const aug_box& b, float x, float y, float z) {
#pragma clang fp contract(off)
    const float ex = x - b.cx, ey = y - b.cy, ez = z - b.zb;
    const float lx = ex * b.c + ey * b.s;
    const float ly = ey * b.c - ex * b.s;
    return __builtin_fabsf(lx) < b.hx && __builtin_fabsf(ly) < b.hy && ez > 0.f && ez < b.dz;
}
