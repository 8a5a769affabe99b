// The device pieces of the contract's 8-bit fixed-point bilinear resize (include/cmt_hip.h,
// cmt_img_resize_prepare) that imgprep.hip and imgaug.hip share: the source coordinate of a resized index, the
// two integer coefficients of its fraction, and the loader of a tap pair's bytes.
#pragma once
#include "cmt_common.h"

struct __attribute__((aligned(4))) img_prep_dw2 { unsigned a, b; };

// floor and the two integer coefficients of resized index d on an axis of scale sc
__device__ __forceinline__ void img_resize_coord(int d, double sc, int& s, float& t) {
#pragma clang fp contract(off)   // __dmul_rn / __dsub_rn are plain operators here and would still fuse
    const double m = ((double)d + 0.5) * sc;
    const float f = (float)(m - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    t = __fsub_rn(f, fl);
}

__device__ __forceinline__ void img_resize_coefs(float t, int& c0, int& c1) {
    c1 = (int)rintf(__fmul_rn(t, 2048.f));
    c0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, t), 2048.f));
}

// the bytes at ap, 6 (PAIR) or 3 of them, as lo = bytes 0..3 and hi = bytes 4..5 (the rest is not used)
template <bool PAIR>
__device__ __forceinline__ void img_resize_taps(const uint8_t* ap, unsigned& lo, unsigned& hi) {
    const unsigned sh = (unsigned)((uintptr_t)ap & 3);
    const unsigned* q = (const unsigned*)(ap - sh);
    unsigned d0, d1, d2 = 0u;
    if (PAIR) {
        const img_prep_dw2 d = *(const img_prep_dw2*)q;   // bytes sh .. sh + 5 reach the second dword at any phase
        d0 = d.a, d1 = d.b;
        if (sh == 3u) d2 = q[2];
    } else {
        d0 = q[0];
        d1 = sh >= 2u ? q[1] : 0u;
    }
    lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
    hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
}

// one channel's byte from the two rows' tap pairs (u, w) with the horizontal (a0, a1) and vertical (b0, b1)
// coefficients: the contract's Hrow >> 4, the two >> 16 products and the rounding >> 2
__device__ __forceinline__ int img_resize_byte(int u0, int w0, int u1, int w1, int a0, int a1, int b0, int b1) {
    const int h0 = (u0 * a0 + w0 * a1) >> 4, h1 = (u1 * a0 + w1 * a1) >> 4;
    return (((b0 * h0) >> 16) + ((b1 * h1) >> 16) + 2) >> 2;
}
