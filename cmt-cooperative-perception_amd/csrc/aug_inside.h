// The inside test of include/cmt_hip.h (points_in_rbbox, the open interior) and the tile / wave helpers that
// ptsaug.hip and gtdb.hip share: both files stage a box and test a point with these instructions, so a point near
// a face falls on the same side in cmt_points_in_boxes, cmt_pts_augment and cmt_gtdb_extract.  Contraction is off
// in the row functions (and for both files, see the Makefile).
#pragma once
#include "cmt_common.h"

#include <cmath>

constexpr int AUG_T = 1024;           // slots (points) per tile
constexpr int AUG_THREADS = 256;
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

__device__ __forceinline__ int aug_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// lanes below this one whose bit is set in a ballot
__device__ __forceinline__ int aug_wave_rank(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ int aug_clamped(const int* word, unsigned n) {
    if (!word) return (int)n;
    const int c = *word;
    return c < 0 ? 0 : ((unsigned)c > n ? (int)n : c);
}

static inline bool aug_aligned(const void* q, uintptr_t a) { return (((uintptr_t)q) & (a - 1)) == 0; }
