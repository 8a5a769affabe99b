// cmt_img_prepare: camera frames as they are loaded (uint8, interleaved [N][Hs][Ws][3]) -> the image
// backbone's input (fp32 planar [N][3][Hp][Wp]) in one pass: integer crop, per-channel normalisation,
// zero padding to the padded size and the HWC -> CHW layout (include/cmt_hip.h).
//
// One thread owns 4 consecutive destination columns of one destination row: 12 source bytes in, one
// 16-byte store per channel plane out (scalar stores where Wp or the destination's alignment forbid).  A
// wave reads 768 contiguous source bytes and writes three 1 KiB runs.  The source row start (3 * x0 and
// 3 * Ws are arbitrary) is not dword-aligned in general: the thread loads the aligned dwords that cover its
// 12 bytes and funnel-shifts them (v_alignbyte_b32), so the loads stay dword loads.  Groups that touch the
// crop's right edge or pixels outside the source take a per-pixel path with byte loads.
#include "cmt_common.h"
#include "img_resize.h"   // img_resize_coord, img_resize_coefs, img_resize_taps

struct img_prep_p {
    const uint8_t* src;
    float* dst;
    int Hs, Ws, x0, y0, w, h, Hp, Wp;
    int G;               // 4-column groups per destination row, ceil(Wp / 4)
    unsigned total;      // N * Hp * G
    int rgb;             // destination channel c reads source channel 2 - c (else c)
    float mean[3], inv[3];
};

struct __attribute__((aligned(4))) img_prep_dw3 { unsigned a, b, c; };

__device__ __forceinline__ unsigned img_prep_byte(const unsigned* wd, int k) { return (wd[k >> 2] >> (8 * (k & 3))) & 0xffu; }

template <bool VEC>
__global__ __launch_bounds__(256) void img_prepare_kernel(img_prep_p p) {
    const unsigned step = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < p.total; i += step) {
        const unsigned row = i / (unsigned)p.G;
        const int g = (int)(i - row * (unsigned)p.G);
        const unsigned n = row / (unsigned)p.Hp;
        const int y = (int)(row - n * (unsigned)p.Hp);
        const int x = 4 * g;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = 0.f;
        if (y < p.h && x < p.w) {
            unsigned wd[3] = {0u, 0u, 0u};   // the group's 12 source bytes, pixels outside the source stay 0
            const int sy = p.y0 + y, sx = p.x0 + x;
            if (sy >= 0 && sy < p.Hs) {
                const uint8_t* rp = p.src + ((int64_t)n * p.Hs + sy) * ((int64_t)p.Ws * 3);
                if (sx >= 0 && sx + 3 < p.Ws && x + 3 < p.w) {
                    const uint8_t* ap = rp + (int64_t)sx * 3;
                    const unsigned sh = (unsigned)((uintptr_t)ap & 3);
                    const unsigned* q = (const unsigned*)(ap - sh);   // pointer arithmetic: stays a global load
                    const img_prep_dw3 d = *(const img_prep_dw3*)q;
                    const unsigned d3 = sh ? q[3] : 0u;   // the fourth dword holds a needed byte only when sh != 0
                    wd[0] = __builtin_amdgcn_alignbyte(d.b, d.a, sh);
                    wd[1] = __builtin_amdgcn_alignbyte(d.c, d.b, sh);
                    wd[2] = __builtin_amdgcn_alignbyte(d3, d.c, sh);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int xs = sx + j;
                        if (x + j < p.w && xs >= 0 && xs < p.Ws) {
                            const uint8_t* px = rp + (int64_t)xs * 3;
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                const int b = 3 * j + k;
                                wd[b >> 2] |= (unsigned)px[k] << (8 * (b & 3));
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned b = p.rgb ? img_prep_byte(wd, 3 * j + 2 - c) : img_prep_byte(wd, 3 * j + c);
                    v[c][j] = (x + j < p.w) ? __fmul_rn(__fsub_rn((float)b, p.mean[c]), p.inv[c]) : 0.f;
                }
        }
        float* o = p.dst + (((int64_t)n * 3) * p.Hp + y) * (int64_t)p.Wp + x;
        const int64_t plane = (int64_t)p.Hp * p.Wp;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (VEC) {
                f32x4 t = {v[c][0], v[c][1], v[c][2], v[c][3]};
                *(f32x4*)(o + c * plane) = t;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < p.Wp) o[c * plane + j] = v[c][j];
            }
        }
    }
}

extern "C" int64_t cmt_img_prepare_args_size(void) { return (int64_t)sizeof(cmt_img_prepare_args); }

extern "C" int cmt_img_prepare(const cmt_img_prepare_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_prepare: null argument struct");
    CMT_REQUIRE(a->src && a->dst, "cmt_img_prepare: src and dst must be non-null");
    CMT_REQUIRE(a->N > 0 && a->Hs > 0 && a->Ws > 0, "cmt_img_prepare: N, Hs and Ws must be positive");
    CMT_REQUIRE(a->w > 0 && a->h > 0, "cmt_img_prepare: the crop's w and h must be positive");
    CMT_REQUIRE(a->Hp >= a->h, "cmt_img_prepare: Hp must be at least the crop's h");
    CMT_REQUIRE(a->Wp >= a->w, "cmt_img_prepare: Wp must be at least the crop's w");
    const int lim = 1 << 30;
    CMT_REQUIRE(a->x0 > -lim && a->x0 < lim && a->y0 > -lim && a->y0 < lim && a->w < lim && a->h < lim &&
                a->Hp < lim && a->Wp < lim, "cmt_img_prepare: crop origin or sizes beyond 2^30");
    CMT_REQUIRE((((uintptr_t)a->dst) & 3) == 0, "cmt_img_prepare: dst must be 4-byte aligned");
    for (int c = 0; c < 3; ++c)
        CMT_REQUIRE(a->mean[c] == a->mean[c] && a->inv_std[c] == a->inv_std[c], "cmt_img_prepare: NaN constant");
    const int G = cdiv(a->Wp, 4);
    const int64_t per_image = (int64_t)a->Hp * G;   // < 2^58
    CMT_REQUIRE(a->N <= (((int64_t)1 << 31) - 1) / per_image, "cmt_img_prepare: N * Hp * ceil(Wp / 4) must be below 2^31");
    const int64_t total = a->N * per_image;
    img_prep_p p;
    p.src = (const uint8_t*)a->src;
    p.dst = (float*)a->dst;
    p.Hs = a->Hs, p.Ws = a->Ws, p.x0 = a->x0, p.y0 = a->y0, p.w = a->w, p.h = a->h, p.Hp = a->Hp, p.Wp = a->Wp;
    p.G = G;
    p.rgb = a->to_rgb ? 1 : 0;
    p.total = (unsigned)total;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = a->mean[c];
        p.inv[c] = a->inv_std[c];
    }
    // memory bound: at most 8 workgroups per CU, the rest of the groups by grid stride
    const int64_t blocks = cdiv64(total, 256);
    const int64_t cap = (int64_t)8 * cmt_cu_count();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
    const bool vec = a->Wp % 4 == 0 && (((uintptr_t)a->dst) & 15) == 0;
    if (vec)
        img_prepare_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    else
        img_prepare_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_img_prepare");
}

// ---- cmt_img_resize_prepare: the same pass with an 8-bit fixed-point bilinear resize in front of the window ----
// The thread shape is cmt_img_prepare's (4 destination columns of one row, one 16-byte store per plane).  A
// destination pixel reads two source rows and, in each, the two horizontal taps: 6 contiguous bytes at an
// arbitrary byte phase, loaded as the aligned dwords that hold them (two, a third only at phase 3) and
// funnel-shifted.  The tap pair is always (s, s + 1) with s <= Ws - 2: the contract's border case s = Ws - 1
// with coefficients (2048, 0) is read as the pair (Ws - 2, Ws - 1) with (0, 2048), the same sum, so the pair
// never reaches past the source row; a source one pixel wide reads 3 bytes.  Tap indices are clamped before
// an address is formed, and a pixel outside the window or outside the resized image forms none.  The source
// coordinate is evaluated as the contract writes it, a float64 multiply and a float64 subtract, with
// contraction switched off for that function: an FMA moves f in rare columns.
struct img_resize_p {
    const uint8_t* src;
    float* dst;
    double sx, sy;       // (double)Ws / Wr, (double)Hs / Hr
    int Hs, Ws, Hr, Wr, x0, y0, w, h, Hp, Wp;
    int G;               // 4-column groups per destination row, ceil(Wp / 4)
    unsigned total;      // N * Hp * G
    int rgb;
    float mean[3], inv[3];
};

template <bool VEC, bool PAIR>
__global__ __launch_bounds__(256) void img_resize_prepare_kernel(img_resize_p p) {
    const unsigned step = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < p.total; i += step) {
        const unsigned row = i / (unsigned)p.G;
        const int g = (int)(i - row * (unsigned)p.G);
        const unsigned n = row / (unsigned)p.Hp;
        const int y = (int)(row - n * (unsigned)p.Hp);
        const int x = 4 * g;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = 0.f;
        if (y < p.h && x < p.w) {
            unsigned px[4] = {0u, 0u, 0u, 0u};   // the resized pixels' 3 bytes, pixels outside the resized image stay 0
            const int ry = p.y0 + y, rx = p.x0 + x;
            if (ry >= 0 && ry < p.Hr) {
                int sy, b0, b1;
                float ty;
                img_resize_coord(ry, p.sy, sy, ty);
                img_resize_coefs(ty, b0, b1);
                const int r0 = min(max(sy, 0), p.Hs - 1), r1 = min(max(sy + 1, 0), p.Hs - 1);
                const int64_t rb = (int64_t)p.Ws * 3;
                const uint8_t* img = p.src + (int64_t)n * p.Hs * rb;
                const uint8_t* rp0 = img + r0 * rb;
                const uint8_t* rp1 = img + r1 * rb;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (x + j < p.w && rx + j >= 0 && rx + j < p.Wr) {
                        int s, a0, a1;
                        float t;
                        img_resize_coord(rx + j, p.sx, s, t);
                        if (s < 0) s = 0, t = 0.f;
                        if (s >= p.Ws - 1) s = p.Ws - 1, t = 0.f;
                        img_resize_coefs(t, a0, a1);
                        if (PAIR && s == p.Ws - 1) s -= 1, a1 = a0, a0 = 0;   // (Ws - 1: 2048, 0) as (Ws - 2: 0, 2048)
                        unsigned lo0, hi0, lo1, hi1;
                        img_resize_taps<PAIR>(rp0 + (int64_t)s * 3, lo0, hi0);
                        img_resize_taps<PAIR>(rp1 + (int64_t)s * 3, lo1, hi1);
                        unsigned o = 0u;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const int u0 = (int)((lo0 >> (8 * k)) & 0xffu), u1 = (int)((lo1 >> (8 * k)) & 0xffu);
                            const int w0 = PAIR ? (int)((k == 0 ? lo0 >> 24 : hi0 >> (8 * (k - 1))) & 0xffu) : 0;
                            const int w1 = PAIR ? (int)((k == 0 ? lo1 >> 24 : hi1 >> (8 * (k - 1))) & 0xffu) : 0;
                            const int h0 = (u0 * a0 + w0 * a1) >> 4, h1 = (u1 * a0 + w1 * a1) >> 4;
                            const int b = (((b0 * h0) >> 16) + ((b1 * h1) >> 16) + 2) >> 2;
                            o |= (unsigned)b << (8 * k);
                        }
                        px[j] = o;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned b = (px[j] >> (8 * (p.rgb ? 2 - c : c))) & 0xffu;
                    v[c][j] = (x + j < p.w) ? __fmul_rn(__fsub_rn((float)b, p.mean[c]), p.inv[c]) : 0.f;
                }
        }
        float* o = p.dst + (((int64_t)n * 3) * p.Hp + y) * (int64_t)p.Wp + x;
        const int64_t plane = (int64_t)p.Hp * p.Wp;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (VEC) {
                f32x4 t = {v[c][0], v[c][1], v[c][2], v[c][3]};
                *(f32x4*)(o + c * plane) = t;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < p.Wp) o[c * plane + j] = v[c][j];
            }
        }
    }
}

extern "C" int64_t cmt_img_resize_args_size(void) { return (int64_t)sizeof(cmt_img_resize_args); }

extern "C" int cmt_img_resize_prepare(const cmt_img_resize_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_resize_prepare: null argument struct");
    CMT_REQUIRE(a->src && a->dst, "cmt_img_resize_prepare: src and dst must be non-null");
    CMT_REQUIRE(a->N > 0 && a->Hs > 0 && a->Ws > 0, "cmt_img_resize_prepare: N, Hs and Ws must be positive");
    CMT_REQUIRE(a->Hr > 0 && a->Wr > 0, "cmt_img_resize_prepare: the resized size Hr, Wr must be positive");
    CMT_REQUIRE(a->w > 0 && a->h > 0, "cmt_img_resize_prepare: the crop's w and h must be positive");
    CMT_REQUIRE(a->Hp >= a->h, "cmt_img_resize_prepare: Hp must be at least the crop's h");
    CMT_REQUIRE(a->Wp >= a->w, "cmt_img_resize_prepare: Wp must be at least the crop's w");
    const int lim = 1 << 30;
    CMT_REQUIRE(a->x0 > -lim && a->x0 < lim && a->y0 > -lim && a->y0 < lim && a->w < lim && a->h < lim &&
                a->Hp < lim && a->Wp < lim && a->Hr < lim && a->Wr < lim && a->Hs < lim && a->Ws < lim,
                "cmt_img_resize_prepare: crop origin or sizes beyond 2^30");
    CMT_REQUIRE((((uintptr_t)a->dst) & 3) == 0, "cmt_img_resize_prepare: dst must be 4-byte aligned");
    for (int c = 0; c < 3; ++c)
        CMT_REQUIRE(a->mean[c] == a->mean[c] && a->inv_std[c] == a->inv_std[c], "cmt_img_resize_prepare: NaN constant");
    const int G = cdiv(a->Wp, 4);
    const int64_t per_image = (int64_t)a->Hp * G;
    CMT_REQUIRE(a->N <= (((int64_t)1 << 31) - 1) / per_image,
                "cmt_img_resize_prepare: N * Hp * ceil(Wp / 4) must be below 2^31");
    const int64_t total = a->N * per_image;
    img_resize_p p;
    p.src = (const uint8_t*)a->src;
    p.dst = (float*)a->dst;
    p.sx = (double)a->Ws / (double)a->Wr;
    p.sy = (double)a->Hs / (double)a->Hr;
    p.Hs = a->Hs, p.Ws = a->Ws, p.Hr = a->Hr, p.Wr = a->Wr;
    p.x0 = a->x0, p.y0 = a->y0, p.w = a->w, p.h = a->h, p.Hp = a->Hp, p.Wp = a->Wp;
    p.G = G;
    p.rgb = a->to_rgb ? 1 : 0;
    p.total = (unsigned)total;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = a->mean[c];
        p.inv[c] = a->inv_std[c];
    }
    const int64_t blocks = cdiv64(total, 256);
    const int64_t cap = (int64_t)8 * cmt_cu_count();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = a->Wp % 4 == 0 && (((uintptr_t)a->dst) & 15) == 0;
    const bool pair = a->Ws > 1;
    if (vec && pair)
        img_resize_prepare_kernel<true, true><<<grid, 256, 0, st>>>(p);
    else if (vec)
        img_resize_prepare_kernel<true, false><<<grid, 256, 0, st>>>(p);
    else if (pair)
        img_resize_prepare_kernel<false, true><<<grid, 256, 0, st>>>(p);
    else
        img_resize_prepare_kernel<false, false><<<grid, 256, 0, st>>>(p);
    return cmt_check_launch("cmt_img_resize_prepare");
}
