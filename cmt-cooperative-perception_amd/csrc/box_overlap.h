// The rotated-box overlap of one pair, one copy for boxiou.hip (cmt_box_iou, cmt_box_nms) and deteval.hip
// (cmt_det_eval_match_iou).  A pair (A, B) is computed in A's own frame: B's footprint becomes a quadrilateral
// around A's axis-aligned rectangle and is clipped against its four half-planes (Sutherland-Hodgman).  The polygon
// has at most 8 vertices; a lane keeps its two ping-pong vertex lists in an LDS slot of its own (2 lists x 8
// vertices x 2 coordinates, laid out [list][vertex][lane] so the 64 lanes of a wave hit 64 banks whatever vertex each
// of them is at): 32 KB for the 256 lanes of a workgroup, nothing in scratch.  Only the owning lane touches a slot,
// so no barrier guards it.  Every product, sum and quotient is rounded on its own, whatever the including file's
// flags.
#pragma once
#include "wave_ops.h"

#include <cmath>

constexpr int BI_THREADS = 256;              // lanes of a workgroup that own a slot
constexpr int BI_VERTS = 8;
constexpr int BI_SLOT = BI_VERTS * BI_THREADS;   // floats of one vertex list over the workgroup

struct bi_box {
    float x, y, hx, hy, c, s, bot, top, area, vol;
    int ok;
};

__device__ __forceinline__ bi_box bi_derive(const float* r, float z_origin) {
#pragma clang fp contract(off)
    const float x = r[0], y = r[1], z = r[2], dx = r[3], dy = r[4], dz = r[5], yaw = r[6];
    bi_box b;
    b.ok = (finite32(x) && finite32(y) && finite32(z) && finite32(dx) && finite32(dy) && finite32(dz) &&
            finite32(yaw) && dx > 0.f && dy > 0.f && dz > 0.f) ? 1 : 0;
    const float yw = b.ok ? yaw : 0.f;
    b.x = x, b.y = y;
    b.hx = dx * 0.5f, b.hy = dy * 0.5f;
    b.s = sinf(yw), b.c = cosf(yw);
    const float off = z_origin * dz;
    b.bot = z - off;
    b.top = b.bot + dz;
    b.area = dx * dy;
    b.vol = b.area * dz;
    return b;
}

__device__ __forceinline__ bi_box bi_none() {
    bi_box b;
    b.x = b.y = b.hx = b.hy = b.c = b.s = b.bot = b.top = b.area = b.vol = 0.f;
    b.ok = 0;
    return b;
}

// One half-plane of Sutherland-Hodgman on the lane's LDS lists.  u is the clipped coordinate, v the other one;
// UPPER: inside is u <= b, else u >= b.  For every edge (p, q) in order: p if it is inside, then the crossing if
// exactly one end is inside (so q.u != p.u).  m < BI_VERTS guards the list whatever the arithmetic does.
template <bool UPPER>
__device__ __forceinline__ int bi_clip(const float* iu, const float* iv, float* ou, float* ov, int n, float b) {
#pragma clang fp contract(off)
    int m = 0;
    if (n <= 0) return 0;
    const float fu = iu[0], fv = iv[0];
    float pu = fu, pv = fv;
    for (int i = 0; i < n; ++i) {
        const bool last = i + 1 >= n;
        const float qu = last ? fu : iu[(i + 1) * BI_THREADS], qv = last ? fv : iv[(i + 1) * BI_THREADS];
        const bool pin = UPPER ? pu <= b : pu >= b, qin = UPPER ? qu <= b : qu >= b;
        if (pin && m < BI_VERTS) {
            ou[m * BI_THREADS] = pu, ov[m * BI_THREADS] = pv;
            ++m;
        }
        if (pin != qin && m < BI_VERTS) {
            const float num = b - pu, den = qu - pu;
            const float t = num / den;
            const float dv = qv - pv;
            const float tv = t * dv;
            ou[m * BI_THREADS] = b, ov[m * BI_THREADS] = pv + tv;
            ++m;
        }
        pu = qu, pv = qv;
    }
    return m;
}

// The overlap of a valid pair: the footprint area and the common height.  px, py: the lane's slot (element
// [list][vertex] at (list * 8 + vertex) * 256).
__device__ __forceinline__ void bi_pair(const bi_box& A, const bi_box& B, float* px, float* py, float& area, float& h) {
#pragma clang fp contract(off)
    const float tx = B.x - A.x, ty = B.y - A.y;
    const float o0 = tx * A.c, o1 = ty * A.s, o2 = ty * A.c, o3 = tx * A.s;
    const float ox = o0 + o1, oy = o2 - o3;
    const float c0 = B.c * A.c, c1 = B.s * A.s, s0 = B.s * A.c, s1 = B.c * A.s;
    const float c = c0 + c1, s = s0 - s1;
    float* x0 = px;
    float* y0 = py;
    float* x1 = px + BI_SLOT;
    float* y1 = py + BI_SLOT;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lx = (k >= 2) ? B.hx : -B.hx, ly = (k == 1 || k == 2) ? B.hy : -B.hy;
        const float a0 = lx * c, a1 = ly * s, b0 = lx * s, b1 = ly * c;
        const float rx = a0 - a1, ry = b0 + b1;
        x0[k * BI_THREADS] = rx + ox;
        y0[k * BI_THREADS] = ry + oy;
    }
    int n = bi_clip<true>(x0, y0, x1, y1, 4, A.hx);
    n = bi_clip<false>(x1, y1, x0, y0, n, -A.hx);
    n = bi_clip<true>(y0, x0, y1, x1, n, A.hy);
    n = bi_clip<false>(y1, x1, y0, x0, n, -A.hy);
    float acc = 0.f;
    if (n >= 3) {
        const float vx = x0[0], vy = y0[0];
        float ax = x0[BI_THREADS] - vx, ay = y0[BI_THREADS] - vy;
        for (int i = 2; i < n; ++i) {
            const float bx = x0[i * BI_THREADS] - vx, by = y0[i * BI_THREADS] - vy;
            const float m0 = ax * by, m1 = ay * bx;
            const float cr = m0 - m1;
            acc = acc + cr;
            ax = bx, ay = by;
        }
    }
    area = __builtin_fabsf(acc) * 0.5f;
    const float top = fminf(A.top, B.top), bot = fmaxf(A.bot, B.bot);
    const float dh = top - bot;
    h = fmaxf(0.f, dh);
}

__device__ __forceinline__ float bi_bev(const bi_box& A, const bi_box& B, float area) {
#pragma clang fp contract(off)
    const float sum = A.area + B.area;
    const float uni = sum - area;
    return area / uni;
}

__device__ __forceinline__ float bi_3d(const bi_box& A, const bi_box& B, float area, float h) {
#pragma clang fp contract(off)
    const float inter = area * h;
    const float sum = A.vol + B.vol;
    const float uni = sum - inter;
    return inter / uni;
}
