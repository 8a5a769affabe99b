// The training-side image pipeline (include/cmt_hip.h): cmt_img_augment (resize, crop, flip, rotation,
// normalisation, pad, GridMask and the modal mask in one pass), cmt_grid_mask (the same mask on a prepared
// batch, in place) and cmt_img_paste (the pixel part of unified_sample, in place on the uint8 frames).
//
// cmt_img_augment keeps cmt_img_prepare's thread shape: one thread owns 4 consecutive destination columns of
// one destination row and stores 16 bytes per channel plane (scalar stores where Wp or the destination's
// alignment forbid).  blockIdx.y is the image, so the per-image parameters are wave-uniform reads of the
// kernel argument.  A destination pixel has up to 4 taps of the flipped crop; a tap whose weight is 0
// contributes exactly 0 and is not read, so the unrotated case (fx = fy = 0) reads one tap per pixel, the
// work of cmt_img_resize_prepare.  The file is built with -ffp-contract=off: the contract's float64 products
// and sums are separate roundings.
#include "cmt_common.h"
#include "img_resize.h"

// ---- GridMask: one predicate for both kernels ------------------------------------------------------------------
struct grid_p {
    int d, l, st_h, st_w, use_h, use_w, mode;
    int hh, ww, oy, ox;   // (int)(1.5 Hp), (int)(1.5 Wp), (hh - Hp) / 2, (ww - Wp) / 2
};

__device__ __forceinline__ bool grid_band(int v, int st, int d, int l, int lim) {
    const int r = v - st;
    return r >= 0 && r / d < lim / d && r % d < l;
}

// m(y, x) of the contract as 0.f or 1.f; rowband is per-row work, hoisted by the callers through grid_row
__device__ __forceinline__ bool grid_row(const grid_p& g, int y) { return g.use_h && grid_band(y + g.oy, g.st_h, g.d, g.l, g.hh); }

__device__ __forceinline__ float grid_value(const grid_p& g, bool rowband, int x) {
    const bool colband = g.use_w && grid_band(x + g.ox, g.st_w, g.d, g.l, g.ww);
    const bool base = !(rowband || colband);
    return (g.mode == 1 ? !base : base) ? 1.f : 0.f;
}

static grid_p grid_fill(const cmt_grid_params& a, int Hp, int Wp) {
    grid_p g;
    g.d = a.d, g.l = a.l, g.st_h = a.st_h, g.st_w = a.st_w;
    g.use_h = a.use_h ? 1 : 0, g.use_w = a.use_w ? 1 : 0, g.mode = a.mode;
    g.hh = (int)(1.5 * (double)Hp), g.ww = (int)(1.5 * (double)Wp);
    g.oy = (g.hh - Hp) / 2, g.ox = (g.ww - Wp) / 2;
    return g;
}

static bool grid_valid(const cmt_grid_params& a) {
    return a.d >= 2 && a.d < (1 << 30) && a.l >= 1 && a.l < a.d && a.st_h >= 0 && a.st_h < a.d && a.st_w >= 0 && a.st_w < a.d;
}

// ---- cmt_img_augment ---------------------------------------------------------------------------------------------
struct img_aug_image_p {
    double iM[6];
    double sx, sy;        // (double)Ws / Wr, (double)Hs / Hr
    int Hr, Wr, x0, y0, flip, zero;
};

struct img_aug_p {
    const uint8_t* src;
    float* dst;
    int Hs, Ws, w, h, Hp, Wp;
    int G;                // 4-column groups per destination row, ceil(Wp / 4)
    unsigned per_image;   // Hp * G
    int rgb, masked;
    float mean[3], inv[3];
    grid_p grid;
    img_aug_image_p img[CMT_IMG_AUG_MAX];
};

// the 3 bytes of resized pixel (ry, rx), inside [0, Hr) x [0, Wr): cmt_img_resize_prepare's arithmetic
template <bool PAIR>
__device__ __forceinline__ unsigned img_aug_resized(const uint8_t* img, int Hs, int Ws, double scx, double scy, int ry, int rx) {
    int sy, b0, b1, s, a0, a1;
    float ty, t;
    img_resize_coord(ry, scy, sy, ty);
    img_resize_coefs(ty, b0, b1);
    const int r0 = min(max(sy, 0), Hs - 1), r1 = min(max(sy + 1, 0), Hs - 1);
    img_resize_coord(rx, scx, s, t);
    if (s < 0) s = 0, t = 0.f;
    if (s >= Ws - 1) s = Ws - 1, t = 0.f;
    img_resize_coefs(t, a0, a1);
    if (PAIR && s == Ws - 1) s -= 1, a1 = a0, a0 = 0;   // (Ws - 1: 2048, 0) as (Ws - 2: 0, 2048)
    const int64_t rb = (int64_t)Ws * 3;
    unsigned lo0, hi0, lo1, hi1;
    img_resize_taps<PAIR>(img + r0 * rb + (int64_t)s * 3, lo0, hi0);
    img_resize_taps<PAIR>(img + r1 * rb + (int64_t)s * 3, lo1, hi1);
    unsigned o = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int u0 = (int)((lo0 >> (8 * k)) & 0xffu), u1 = (int)((lo1 >> (8 * k)) & 0xffu);
        const int w0 = PAIR ? (int)((k == 0 ? lo0 >> 24 : hi0 >> (8 * (k - 1))) & 0xffu) : 0;
        const int w1 = PAIR ? (int)((k == 0 ? lo1 >> 24 : hi1 >> (8 * (k - 1))) & 0xffu) : 0;
        o |= (unsigned)img_resize_byte(u0, w0, u1, w1, a0, a1, b0, b1) << (8 * k);
    }
    return o;
}

// the weighted tap sums (1024 * val) of destination pixel (y, x), source channel order; BX, BY are the row's
template <bool PAIR>
__device__ __forceinline__ void img_aug_pixel(const img_aug_p& p, const img_aug_image_p& im, const uint8_t* img,
                                              int64_t BX, int64_t BY, int x, int (&sum)[3]) {
    const int64_t AX = (int64_t)rint(im.iM[0] * (double)x * 1024.0);
    const int64_t AY = (int64_t)rint(im.iM[3] * (double)x * 1024.0);
    const int64_t X = (BX + AX) >> 5, Y = (BY + AY) >> 5;
    const int64_t ix = X >> 5, iy = Y >> 5;
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    sum[0] = sum[1] = sum[2] = 0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int wgt = ((k & 1) ? fx : 32 - fx) * ((k & 2) ? fy : 32 - fy);
        const int64_t tx = ix + (k & 1), ty = iy + (k >> 1);
        if (wgt == 0 || tx < 0 || tx >= p.w || ty < 0 || ty >= p.h) continue;
        const int txf = im.flip ? p.w - 1 - (int)tx : (int)tx;
        const int ry = im.y0 + (int)ty, rx = im.x0 + txf;   // |x0|, |y0|, w, h < 2^30
        if (ry < 0 || ry >= im.Hr || rx < 0 || rx >= im.Wr) continue;
        const unsigned b = img_aug_resized<PAIR>(img, p.Hs, p.Ws, im.sx, im.sy, ry, rx);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += wgt * (int)((b >> (8 * c)) & 0xffu);
    }
}

template <bool VEC, bool PAIR>
__global__ __launch_bounds__(256) void img_augment_kernel(img_aug_p p) {
    const unsigned n = blockIdx.y;
    const img_aug_image_p& im = p.img[n];
    const uint8_t* img = p.src + (int64_t)n * p.Hs * ((int64_t)p.Ws * 3);
    const int64_t plane = (int64_t)p.Hp * p.Wp;
    const unsigned step = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < p.per_image; i += step) {
        const int y = (int)(i / (unsigned)p.G);
        const int x = 4 * (int)(i - (unsigned)y * (unsigned)p.G);
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = 0.f;
        if (y < p.h && x < p.w) {
            const int64_t BX = (int64_t)rint((im.iM[1] * (double)y + im.iM[2]) * 1024.0) + 16;
            const int64_t BY = (int64_t)rint((im.iM[4] * (double)y + im.iM[5]) * 1024.0) + 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (x + j < p.w) {
                    int sum[3] = {0, 0, 0};
                    if (!im.zero) img_aug_pixel<PAIR>(p, im, img, BX, BY, x + j, sum);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float val = (float)sum[p.rgb ? 2 - c : c] * (1.f / 1024.f);   // exact: sum < 2^18
                        v[c][j] = __fmul_rn(__fsub_rn(val, p.mean[c]), p.inv[c]);
                    }
                }
            }
        }
        if (p.masked) {
            const bool rowband = grid_row(p.grid, y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float m = grid_value(p.grid, rowband, x + j);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j] = __fmul_rn(v[c][j], m);
            }
        }
        float* o = p.dst + (((int64_t)n * 3) * p.Hp + y) * (int64_t)p.Wp + x;
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

extern "C" int64_t cmt_img_augment_args_size(void) { return (int64_t)sizeof(cmt_img_augment_args); }

extern "C" int cmt_img_augment(const cmt_img_augment_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_augment: null argument struct");
    CMT_REQUIRE(a->src && a->dst, "cmt_img_augment: src and dst must be non-null");
    CMT_REQUIRE(a->N >= 1 && a->N <= CMT_IMG_AUG_MAX, "cmt_img_augment: N must be in 1..CMT_IMG_AUG_MAX");
    CMT_REQUIRE(a->Hs > 0 && a->Ws > 0, "cmt_img_augment: Hs and Ws must be positive");
    CMT_REQUIRE(a->w > 0 && a->h > 0, "cmt_img_augment: the crop's w and h must be positive");
    CMT_REQUIRE(a->Hp >= a->h, "cmt_img_augment: Hp must be at least the crop's h");
    CMT_REQUIRE(a->Wp >= a->w, "cmt_img_augment: Wp must be at least the crop's w");
    const int lim = 1 << 30;
    CMT_REQUIRE(a->Hs < lim && a->Ws < lim && a->w < lim && a->h < lim && a->Hp < lim && a->Wp < lim,
                "cmt_img_augment: sizes beyond 2^30");
    CMT_REQUIRE((((uintptr_t)a->dst) & 3) == 0, "cmt_img_augment: dst must be 4-byte aligned");
    for (int c = 0; c < 3; ++c)
        CMT_REQUIRE(a->mean[c] == a->mean[c] && a->inv_std[c] == a->inv_std[c], "cmt_img_augment: NaN constant");
    const int G = cdiv(a->Wp, 4);
    const int64_t per_image = (int64_t)a->Hp * G;
    CMT_REQUIRE(per_image < ((int64_t)1 << 31), "cmt_img_augment: Hp * ceil(Wp / 4) must be below 2^31");
    for (int n = 0; n < a->N; ++n) {
        const cmt_img_aug_image& im = a->img[n];
        CMT_REQUIRE(im.Hr > 0 && im.Wr > 0 && im.Hr < lim && im.Wr < lim,
                    "cmt_img_augment: an image's resized size Hr, Wr must be positive and below 2^30");
        CMT_REQUIRE(im.x0 > -lim && im.x0 < lim && im.y0 > -lim && im.y0 < lim, "cmt_img_augment: a crop origin beyond 2^30");
        for (int k = 0; k < 6; ++k)
            CMT_REQUIRE(std::isfinite(im.iM[k]) && std::fabs(im.iM[k]) < 1048576.0,
                        "cmt_img_augment: iM must be finite and below 2^20 in magnitude");
    }
    CMT_REQUIRE(a->grid.d >= 0, "cmt_img_augment: grid.d must not be negative");
    if (a->grid.d > 0)
        CMT_REQUIRE(grid_valid(a->grid), "cmt_img_augment: grid needs 2 <= d < 2^30, 1 <= l < d and 0 <= st_h, st_w < d");
    img_aug_p p;
    p.src = (const uint8_t*)a->src;
    p.dst = (float*)a->dst;
    p.Hs = a->Hs, p.Ws = a->Ws, p.w = a->w, p.h = a->h, p.Hp = a->Hp, p.Wp = a->Wp;
    p.G = G;
    p.per_image = (unsigned)per_image;
    p.rgb = a->to_rgb ? 1 : 0;
    p.masked = a->grid.d > 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = a->mean[c];
        p.inv[c] = a->inv_std[c];
    }
    cmt_grid_params one = a->grid;
    if (!p.masked) one.d = 2, one.l = 1, one.st_h = one.st_w = 0;   // not read by the kernel
    p.grid = grid_fill(one, a->Hp, a->Wp);
    for (int n = 0; n < CMT_IMG_AUG_MAX; ++n) {
        const cmt_img_aug_image& im = a->img[n < a->N ? n : 0];
        img_aug_image_p& q = p.img[n];
        for (int k = 0; k < 6; ++k) q.iM[k] = im.iM[k];
        q.sx = (double)a->Ws / (double)im.Wr;
        q.sy = (double)a->Hs / (double)im.Hr;
        q.Hr = im.Hr, q.Wr = im.Wr, q.x0 = im.x0, q.y0 = im.y0, q.flip = im.flip ? 1 : 0, q.zero = im.zero ? 1 : 0;
    }
    // memory bound: at most 8 workgroups per CU over the N images, the rest of the groups by grid stride
    const int64_t blocks = cdiv64(per_image, 256);
    const int64_t cap = std::max<int64_t>(1, (int64_t)8 * cmt_cu_count() / a->N);
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap), (unsigned)a->N);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = a->Wp % 4 == 0 && (((uintptr_t)a->dst) & 15) == 0;
    const bool pair = a->Ws > 1;
    if (vec && pair)
        img_augment_kernel<true, true><<<grid, 256, 0, st>>>(p);
    else if (vec)
        img_augment_kernel<true, false><<<grid, 256, 0, st>>>(p);
    else if (pair)
        img_augment_kernel<false, true><<<grid, 256, 0, st>>>(p);
    else
        img_augment_kernel<false, false><<<grid, 256, 0, st>>>(p);
    return cmt_check_launch("cmt_img_augment");
}

// ---- cmt_grid_mask -----------------------------------------------------------------------------------------------
struct grid_mask_p {
    float* x;
    int h, w, G;
    unsigned total;   // planes * h * G
    grid_p grid;
};

template <bool VEC>
__global__ __launch_bounds__(256) void grid_mask_kernel(grid_mask_p p) {
    const unsigned step = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < p.total; i += step) {
        const unsigned row = i / (unsigned)p.G;
        const int x = 4 * (int)(i - row * (unsigned)p.G);
        const int y = (int)(row % (unsigned)p.h);
        const bool rowband = grid_row(p.grid, y);
        float* o = p.x + (int64_t)row * p.w + x;
        if (VEC) {
            f32x4 t = *(const f32x4*)o;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = __fmul_rn(t[j], grid_value(p.grid, rowband, x + j));
            *(f32x4*)o = t;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < p.w) o[j] = __fmul_rn(o[j], grid_value(p.grid, rowband, x + j));
        }
    }
}

extern "C" int64_t cmt_grid_mask_args_size(void) { return (int64_t)sizeof(cmt_grid_mask_args); }

extern "C" int cmt_grid_mask(const cmt_grid_mask_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_grid_mask: null argument struct");
    CMT_REQUIRE(a->x != nullptr, "cmt_grid_mask: x must be non-null");
    CMT_REQUIRE((((uintptr_t)a->x) & 3) == 0, "cmt_grid_mask: x must be 4-byte aligned");
    CMT_REQUIRE(a->planes > 0 && a->h > 0 && a->w > 0, "cmt_grid_mask: planes, h and w must be positive");
    CMT_REQUIRE(a->h < (1 << 30) && a->w < (1 << 30), "cmt_grid_mask: h or w beyond 2^30");
    const int G = cdiv(a->w, 4);
    const int64_t per_plane = (int64_t)a->h * G;
    CMT_REQUIRE(a->planes <= (((int64_t)1 << 31) - 1) / per_plane, "cmt_grid_mask: planes * h * ceil(w / 4) must be below 2^31");
    CMT_REQUIRE(grid_valid(a->grid), "cmt_grid_mask: grid needs 2 <= d < 2^30, 1 <= l < d and 0 <= st_h, st_w < d");
    grid_mask_p p;
    p.x = (float*)a->x;
    p.h = a->h, p.w = a->w, p.G = G;
    p.total = (unsigned)(a->planes * per_plane);
    p.grid = grid_fill(a->grid, a->h, a->w);
    const int64_t blocks = cdiv64((int64_t)p.total, 256);
    const int64_t cap = (int64_t)8 * cmt_cu_count();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
    const bool vec = a->w % 4 == 0 && (((uintptr_t)a->x) & 15) == 0;
    if (vec)
        grid_mask_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    else
        grid_mask_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_grid_mask");
}

// ---- cmt_img_paste -----------------------------------------------------------------------------------------------
// One launch for all cameras: blockIdx.y is the camera, blockIdx.x a 64 x 4 pixel tile of the bounding rectangle of
// that camera's list (taken from the host table; a camera with fewer tiles than the widest lets the surplus
// workgroups leave at once).  A wave owns 64 consecutive pixels of one row, 192 contiguous bytes.  The
// workgroup stages the camera's list in LDS, each entry joined with its patch and checked again (a device entry
// that fails a host-side condition becomes an empty rectangle); every thread then walks the staged list in
// order with its pixel in registers and writes the pixel back if a rectangle held it.
constexpr int PASTE_TW = 64, PASTE_TH = 4;

struct paste_entry {
    int x0, y0, x1, y1;
    int kind;             // 0 raw box, 1 sampled box; -1 skipped
    int hc, wc;
    int64_t offset;
    double sx, sy;        // (double)wc / (x1 - x0), (double)hc / (y1 - y0)
};

struct img_paste_p {
    uint8_t* frames;
    const cmt_paste_rect* rects;
    const cmt_paste_patch* patches;
    const uint8_t* patch_bytes;
    int64_t patch_bytes_size;
    double m, om;
    int Hs, Ws, n_patches, mix;
    int count[CMT_IMG_AUG_MAX];
    int bx0[CMT_IMG_AUG_MAX], by0[CMT_IMG_AUG_MAX], bx1[CMT_IMG_AUG_MAX], by1[CMT_IMG_AUG_MAX];
};

// the 3 bytes of the patch resized to rh x rw at (ry, rx), byte loads (a patch has any alignment and no slack)
__device__ __forceinline__ void paste_sample(const uint8_t* pb, int hc, int wc, double scx, double scy, int ry, int rx, int (&c)[3]) {
    int sy, b0, b1, s, a0, a1;
    float ty, t;
    img_resize_coord(ry, scy, sy, ty);
    img_resize_coefs(ty, b0, b1);
    const int r0 = min(max(sy, 0), hc - 1), r1 = min(max(sy + 1, 0), hc - 1);
    img_resize_coord(rx, scx, s, t);
    if (s < 0) s = 0, t = 0.f;
    if (s >= wc - 1) s = wc - 1, t = 0.f;
    img_resize_coefs(t, a0, a1);
    const int s1 = min(s + 1, wc - 1);
    const uint8_t* p00 = pb + ((int64_t)r0 * wc + s) * 3;
    const uint8_t* p01 = pb + ((int64_t)r0 * wc + s1) * 3;
    const uint8_t* p10 = pb + ((int64_t)r1 * wc + s) * 3;
    const uint8_t* p11 = pb + ((int64_t)r1 * wc + s1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = img_resize_byte(p00[k], p01[k], p10[k], p11[k], a0, a1, b0, b1);
}

__global__ __launch_bounds__(256) void img_paste_kernel(img_paste_p p) {
    __shared__ paste_entry list[CMT_PASTE_MAX_RECTS];
    const int n = blockIdx.y;
    const int bx0 = p.bx0[n], by0 = p.by0[n], bx1 = p.bx1[n], by1 = p.by1[n];
    const int tiles_x = (bx1 - bx0 + PASTE_TW - 1) / PASTE_TW, tiles_y = (by1 - by0 + PASTE_TH - 1) / PASTE_TH;
    if (blockIdx.x >= (unsigned)tiles_x * (unsigned)tiles_y) return;   // uniform over the workgroup
    const int count = min(p.count[n], CMT_PASTE_MAX_RECTS);
    for (int i = threadIdx.x; i < count; i += 256) {
        const cmt_paste_rect r = p.rects[(int64_t)n * CMT_PASTE_MAX_RECTS + i];
        paste_entry e;
        e.x0 = r.x0, e.y0 = r.y0, e.x1 = r.x1, e.y1 = r.y1;
        e.kind = -1, e.hc = 0, e.wc = 0, e.offset = 0, e.sx = 0.0, e.sy = 0.0;
        const bool inside = r.x0 >= 0 && r.y0 >= 0 && r.x0 < r.x1 && r.y0 < r.y1 && r.x1 <= p.Ws && r.y1 <= p.Hs;
        if (inside && r.crop == -1) e.kind = 0;
        if (inside && r.crop >= 0 && r.crop < p.n_patches) {
            const cmt_paste_patch t = p.patches[r.crop];
            if (t.hc > 0 && t.wc > 0 && t.hc < 32768 && t.wc < 32768 && t.offset >= 0 &&
                t.offset + (int64_t)3 * t.hc * t.wc <= p.patch_bytes_size) {
                e.kind = 1, e.hc = t.hc, e.wc = t.wc, e.offset = t.offset;
                e.sx = (double)t.wc / (double)(r.x1 - r.x0);
                e.sy = (double)t.hc / (double)(r.y1 - r.y0);
            }
        }
        list[i] = e;
    }
    __syncthreads();
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x = bx0 + tx * PASTE_TW + (int)(threadIdx.x & 63), y = by0 + ty * PASTE_TH + (int)(threadIdx.x >> 6);
    if (x >= bx1 || y >= by1) return;   // the bounding rectangle lies inside the frame (checked on the host)
    uint8_t* px = p.frames + (((int64_t)n * p.Hs + y) * p.Ws + x) * 3;
    int v[3];
    bool held = false;
    bool loaded = false;
    for (int i = 0; i < count; ++i) {
        const paste_entry& e = list[i];
        if (e.kind < 0 || x < e.x0 || x >= e.x1 || y < e.y0 || y >= e.y1) continue;
        if (!loaded) {
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = px[k];
            loaded = true;
        }
        if (e.kind == 0) {
            if (p.mix) {
#pragma unroll
                for (int k = 0; k < 3; ++k) v[k] = (int)((double)v[k] * p.om + (double)v[k] * p.m);
                held = true;
            }
        } else {
            int c[3];
            paste_sample(p.patch_bytes + e.offset, e.hc, e.wc, e.sx, e.sy, y - e.y0, x - e.x0, c);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = p.mix ? (int)((double)v[k] * p.om + (double)c[k] * p.m) : c[k];
            held = true;
        }
    }
    if (held) {
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = (uint8_t)v[k];
    }
}

extern "C" int64_t cmt_img_paste_args_size(void) { return (int64_t)sizeof(cmt_img_paste_args); }

extern "C" int cmt_img_paste(const cmt_img_paste_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_paste: null argument struct");
    CMT_REQUIRE(a->frames != nullptr, "cmt_img_paste: frames must be non-null");
    CMT_REQUIRE(a->N >= 1 && a->N <= CMT_IMG_AUG_MAX, "cmt_img_paste: N must be in 1..CMT_IMG_AUG_MAX");
    const int lim = 1 << 30;
    CMT_REQUIRE(a->Hs > 0 && a->Ws > 0 && a->Hs < lim && a->Ws < lim, "cmt_img_paste: Hs and Ws must be positive and below 2^30");
    CMT_REQUIRE(a->n_patches >= 0, "cmt_img_paste: n_patches must not be negative");
    CMT_REQUIRE(a->mixup == a->mixup && a->mixup <= 1.0, "cmt_img_paste: mixup must be at most 1 (negative: plain paste), not NaN");
    int64_t total = 0;
    for (int n = 0; n < a->N; ++n) {
        CMT_REQUIRE(a->count[n] >= 0 && a->count[n] <= CMT_PASTE_MAX_RECTS,
                    "cmt_img_paste: a camera's rectangle count must be in 0..CMT_PASTE_MAX_RECTS");
        total += a->count[n];
    }
    if (total > 0) CMT_REQUIRE(a->rects && a->rects_dev, "cmt_img_paste: rects and rects_dev must be non-null");
    if (a->n_patches > 0)
        CMT_REQUIRE(a->patches && a->patches_dev && a->patch_bytes && a->patch_bytes_size >= 0,
                    "cmt_img_paste: patches, patches_dev and patch_bytes must be non-null with n_patches > 0");
    for (int i = 0; i < a->n_patches; ++i) {
        const cmt_paste_patch& t = a->patches[i];
        CMT_REQUIRE(t.hc >= 0 && t.wc >= 0 && t.hc < 32768 && t.wc < 32768, "cmt_img_paste: a patch's hc, wc must be in [0, 2^15)");
        CMT_REQUIRE(t.offset >= 0 && t.offset <= a->patch_bytes_size &&
                    (int64_t)3 * t.hc * t.wc <= a->patch_bytes_size - t.offset,
                    "cmt_img_paste: a patch lies outside patch_bytes");
    }
    img_paste_p p;
    int64_t max_tiles = 0;
    for (int n = 0; n < CMT_IMG_AUG_MAX; ++n) {
        p.count[n] = n < a->N ? a->count[n] : 0;
        int bx0 = a->Ws, by0 = a->Hs, bx1 = 0, by1 = 0;
        for (int i = 0; i < p.count[n]; ++i) {
            const cmt_paste_rect& r = a->rects[(int64_t)n * CMT_PASTE_MAX_RECTS + i];
            CMT_REQUIRE(r.x0 >= 0 && r.y0 >= 0 && r.x0 <= r.x1 && r.y0 <= r.y1 && r.x1 <= a->Ws && r.y1 <= a->Hs,
                        "cmt_img_paste: a rectangle must satisfy 0 <= x0 <= x1 <= Ws and 0 <= y0 <= y1 <= Hs");
            CMT_REQUIRE(r.crop >= -1 && r.crop < a->n_patches, "cmt_img_paste: a rectangle's crop must be -1 or a patch index");
            if (r.x0 < r.x1 && r.y0 < r.y1) {
                bx0 = std::min(bx0, r.x0), by0 = std::min(by0, r.y0), bx1 = std::max(bx1, r.x1), by1 = std::max(by1, r.y1);
            }
        }
        if (bx1 <= bx0 || by1 <= by0) bx0 = by0 = bx1 = by1 = 0, p.count[n] = 0;
        p.bx0[n] = bx0, p.by0[n] = by0, p.bx1[n] = bx1, p.by1[n] = by1;
        const int64_t tiles = cdiv64(bx1 - bx0, PASTE_TW) * cdiv64(by1 - by0, PASTE_TH);
        CMT_REQUIRE(tiles < ((int64_t)1 << 31), "cmt_img_paste: a camera's bounding rectangle has 2^31 or more tiles");
        max_tiles = std::max(max_tiles, tiles);
    }
    if (max_tiles == 0) return CMT_OK;   // nothing to paste
    p.frames = (uint8_t*)a->frames;
    p.rects = (const cmt_paste_rect*)a->rects_dev;
    p.patches = (const cmt_paste_patch*)a->patches_dev;
    p.patch_bytes = (const uint8_t*)a->patch_bytes;
    p.patch_bytes_size = a->n_patches > 0 ? a->patch_bytes_size : 0;
    p.mix = a->mixup >= 0.0 ? 1 : 0;
    p.m = a->mixup;
    p.om = 1.0 - a->mixup;
    p.Hs = a->Hs, p.Ws = a->Ws, p.n_patches = a->n_patches;
    const dim3 grid((unsigned)max_tiles, (unsigned)a->N);
    img_paste_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_img_paste");
}
