// Result pictures of include/cmt_hip.h on the device (cmt_render_*): points, segments, box wire frames and decimal
// numbers drawn into a uint64 key plane, and the plane resolved to uint8 pictures.
//
// Every drawing kernel only does 64-bit atomic maxima on the plane with key = layer << 56 | order << 24 | rgb.  Maximum
// is commutative and idempotent, so the plane does not depend on the order of launches, waves or writers: the
// pictures are bitwise repeatable with no ordering machinery.  The segment (near clip, projection, Liang-Barsky, the
// integer walk) exists once, rd_segment, and is shared by the segment and the box kernels: one wave per (item, view),
// the lanes across the walk.  A wave's clip arithmetic is uniform over its lanes.
// The file is built with -ffp-contract=off: every product, sum and quotient of the contract is rounded on its own.
#include "box_overlap.h"
#include "wave_ops.h"

#include <cmath>

typedef unsigned long long u64;

constexpr int RD_THREADS = 256;
constexpr int RD_WAVES = RD_THREADS / 64;

struct rd_target {
    u64* plane;
    int V, H, W;
    unsigned layer;
    float near;
    float view[CMT_RENDER_MAX_VIEWS][16];
};

__device__ __forceinline__ unsigned rd_okey(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

__device__ __forceinline__ u64 rd_key(unsigned layer, unsigned order, unsigned rgb) {
    return ((u64)layer << 56) | ((u64)order << 24) | (u64)(rgb & 0xFFFFFFu);
}

// the only write of the drawing kernels; (X, Y) outside the picture is not written
__device__ __forceinline__ void rd_put(const rd_target& t, int v, int X, int Y, u64 key) {
    if (X < 0 || X >= t.W || Y < 0 || Y >= t.H) return;
    u64* q = t.plane + ((int64_t)v * t.H + Y) * t.W + X;
    __hip_atomic_fetch_max(q, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// row r of a scene position in view v
__device__ __forceinline__ float rd_row(const rd_target& t, int v, int r, float x, float y, float z) {
#pragma clang fp contract(off)
    const float* m = t.view[v] + 4 * r;
    const float a = m[0] * x, b = m[1] * y, c = m[2] * z;
    const float ab = a + b;
    const float abc = ab + c;
    return abc + m[3];
}

// floor(f) clamped to [lo, hi] on the floats; f is finite
__device__ __forceinline__ int rd_floor_clamp(float f, float lo, float hi) {
    return (int)fminf(fmaxf(floorf(f), lo), hi);
}

__device__ __forceinline__ int rd_floordiv(int a, int b) {   // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// THE SEGMENT of the contract, for one wave: every lane passes the same ends.  a, b: 3 floats (2 when planar).
__device__ __forceinline__ void rd_segment(const rd_target& t, int v, bool planar, const float* a, const float* b,
                                           int thick, u64 key, int lane) {
#pragma clang fp contract(off)
    float ua, va, ub, vb;
    if (planar) {
        ua = a[0], va = a[1], ub = b[0], vb = b[1];
    } else {
        if (!(finite32(a[0]) && finite32(a[1]) && finite32(a[2]) && finite32(b[0]) && finite32(b[1]) && finite32(b[2])))
            return;
        float A[4], B[4];
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            A[r] = rd_row(t, v, r, a[0], a[1], a[2]);
            B[r] = rd_row(t, v, r, b[0], b[1], b[2]);
            fin = fin && finite32(A[r]) && finite32(B[r]);
        }
        if (!fin) return;
        const bool ina = A[3] >= t.near, inb = B[3] >= t.near;
        if (!ina && !inb) return;
        if (ina != inb) {
            const float num = t.near - A[3], den = B[3] - A[3];
            const float tc = num / den;
            const float d0 = B[0] - A[0], d1 = B[1] - A[1];
            const float e0 = tc * d0, e1 = tc * d1;
            const float c0 = A[0] + e0, c1 = A[1] + e1;
            if (ina) B[0] = c0, B[1] = c1, B[3] = t.near;
            else A[0] = c0, A[1] = c1, A[3] = t.near;
        }
        ua = A[0] / A[3], va = A[1] / A[3], ub = B[0] / B[3], vb = B[1] / B[3];
    }
    const float dx = ub - ua, dy = vb - va;
    if (!(finite32(ua) && finite32(va) && finite32(ub) && finite32(vb) && finite32(dx) && finite32(dy))) return;
    const float xmax = (float)(t.W + 1), ymax = (float)(t.H + 1);
    float t0 = 0.f, t1 = 1.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float p = e == 0 ? -dx : (e == 1 ? dx : (e == 2 ? -dy : dy));
        const float q = e == 0 ? ua - (-1.f) : (e == 1 ? xmax - ua : (e == 2 ? va - (-1.f) : ymax - va));
        if (p == 0.f) {
            if (q < 0.f) return;
            continue;
        }
        const float r = q / p;
        if (p < 0.f) {
            if (r > t1) return;
            if (r > t0) t0 = r;
        } else {
            if (r < t0) return;
            if (r < t1) t1 = r;
        }
    }
    float xa = ua, ya = va, xb = ub, yb = vb;
    if (t0 > 0.f) {
        const float sx = t0 * dx, sy = t0 * dy;
        xa = ua + sx, ya = va + sy;
    }
    if (t1 < 1.f) {
        const float sx = t1 * dx, sy = t1 * dy;
        xb = ua + sx, yb = va + sy;
    }
    const float cx = (float)(t.W + 2), cy = (float)(t.H + 2);
    const int X0 = rd_floor_clamp(xa, -2.f, cx), Y0 = rd_floor_clamp(ya, -2.f, cy);
    const int X1 = rd_floor_clamp(xb, -2.f, cx), Y1 = rd_floor_clamp(yb, -2.f, cy);
    const int dX = X1 - X0, dY = Y1 - Y0;
    const int adx = dX < 0 ? -dX : dX, ady = dY < 0 ? -dY : dY;
    const int n = adx > ady ? adx : ady;          // <= 4100: 2 * dX * k + n stays below 2^26
    const int lo = -((thick - 1) / 2), hi = thick / 2;
    for (int k = lane; k <= n; k += 64) {
        int X = X0, Y = Y0;
        if (n > 0) {
            X += rd_floordiv(2 * dX * k + n, 2 * n);
            Y += rd_floordiv(2 * dY * k + n, 2 * n);
        }
        for (int j = lo; j <= hi; ++j)
            for (int i = lo; i <= hi; ++i) rd_put(t, v, X + i, Y + j, key);
    }
}

// ---- cmt_render_points -----------------------------------------------------------------------------------------
struct rd_points_p {
    rd_target t;
    const float* points;
    const int* n;
    const unsigned* lut;
    int N, ld, radius, near_wins, color_col;
    float lo, inv_span;
};

__global__ __launch_bounds__(RD_THREADS) void render_points_kernel(rd_points_p p) {
#pragma clang fp contract(off)
    const int n = clamp_count(p.n, p.N);
    const int64_t stride = (int64_t)gridDim.x * RD_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x; i < n; i += stride) {
        const float* r = p.points + i * p.ld;
        const float x = r[0], y = r[1], z = r[2];
        if (!(finite32(x) && finite32(y) && finite32(z))) continue;
        const float col = p.color_col >= 0 ? r[p.color_col] : 0.f;
        for (int v = 0; v < p.t.V; ++v) {
            const float r3 = rd_row(p.t, v, 3, x, y, z);
            if (!(r3 >= p.t.near)) continue;
            const float r0 = rd_row(p.t, v, 0, x, y, z), r1 = rd_row(p.t, v, 1, x, y, z), d = rd_row(p.t, v, 2, x, y, z);
            const float pu = r0 / r3, pv = r1 / r3;
            if (!finite32(d) || !(pu >= 0.f && pu < (float)p.t.W && pv >= 0.f && pv < (float)p.t.H)) continue;
            const int X = (int)floorf(pu), Y = (int)floorf(pv);
            const float c = p.color_col >= 0 ? col : d;
            const float c0 = c - p.lo;
            const float c1 = c0 * p.inv_span;
            const float tt = c1 * 255.f;
            const int idx = tt >= 255.f ? 255 : (tt >= 0.f ? (int)floorf(tt) : 0);
            const unsigned ok = rd_okey(d);
            const u64 key = rd_key(p.t.layer, p.near_wins ? ~ok : ok, p.lut[idx]);
            for (int j = -p.radius; j <= p.radius; ++j)
                for (int e = -p.radius; e <= p.radius; ++e) rd_put(p.t, v, X + e, Y + j, key);
        }
    }
}

// ---- cmt_render_segments ---------------------------------------------------------------------------------------
struct rd_segments_p {
    rd_target t;
    const float* p0;
    const float* p1;
    const unsigned* rgb;
    const int* rank;
    const int* n;
    int S, planar, thick;
};

__global__ __launch_bounds__(RD_THREADS) void render_segments_kernel(rd_segments_p p) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * RD_WAVES + ((int)threadIdx.x >> 6);
    const int s = (int)(w / p.t.V), v = (int)(w % p.t.V);
    if (s >= clamp_count(p.n, p.S)) return;
    const int c = p.planar ? 2 : 3;
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    for (int e = 0; e < c; ++e) a[e] = p.p0[(int64_t)s * c + e], b[e] = p.p1[(int64_t)s * c + e];
    int rank = p.rank ? p.rank[s] : s;
    if (rank < 0) rank = 0;
    rd_segment(p.t, v, p.planar != 0, a, b, p.thick, rd_key(p.t.layer, 0xFFFFFFFFu - (unsigned)rank, p.rgb[s]), lane);
}

// ---- cmt_render_boxes ------------------------------------------------------------------------------------------
struct rd_boxes_p {
    rd_target t;
    const float* boxes;
    const int* count;
    const int* labels;
    const float* scores;
    const unsigned* class_rgb;
    int M, ld, thick, ncls;
    float z_origin, score_thr;
    unsigned rgb_default;
};

__global__ __launch_bounds__(RD_THREADS) void render_boxes_kernel(rd_boxes_p p) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * RD_WAVES + ((int)threadIdx.x >> 6);
    const int m = (int)(w / p.t.V), v = (int)(w % p.t.V);
    if (m >= clamp_count(p.count, p.M)) return;
    if (p.scores && !(p.scores[m] > p.score_thr)) return;
    const bi_box B = bi_derive(p.boxes + (int64_t)m * p.ld, p.z_origin);
    if (!B.ok) return;
    unsigned rgb = p.rgb_default;
    if (p.labels && p.class_rgb) {
        const int lab = p.labels[m];
        if (lab >= 0 && lab < p.ncls) rgb = p.class_rgb[lab];
    }
    const u64 key = rd_key(p.t.layer, 0xFFFFFFFFu - (unsigned)m, rgb);
    float X[4], Y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lx = (k >= 2) ? B.hx : -B.hx, ly = (k == 1 || k == 2) ? B.hy : -B.hy;
        const float a0 = lx * B.c, a1 = ly * B.s, b0 = lx * B.s, b1 = ly * B.c;
        const float rx = a0 - a1, ry = b0 + b1;
        X[k] = rx + B.x, Y[k] = ry + B.y;
    }
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const float lo0[3] = {X[k], Y[k], B.bot}, lo1[3] = {X[k1], Y[k1], B.bot};
        const float hi0[3] = {X[k], Y[k], B.top}, hi1[3] = {X[k1], Y[k1], B.top};
        rd_segment(p.t, v, false, lo0, lo1, p.thick, key, lane);
        rd_segment(p.t, v, false, hi0, hi1, p.thick, key, lane);
        rd_segment(p.t, v, false, lo0, hi0, p.thick, key, lane);
    }
    const float fc = B.hx * B.c, fs = B.hx * B.s;
    const float h0[3] = {B.x, B.y, B.top}, h1[3] = {fc + B.x, fs + B.y, B.top};
    rd_segment(p.t, v, false, h0, h1, p.thick, key, lane);
}

// ---- cmt_render_digits -----------------------------------------------------------------------------------------
struct rd_digits_p {
    rd_target t;
    const int* values;
    const float* anchors;
    const unsigned* rgb;
    const int* rank;
    int M, planar, scale;
    unsigned rgb_one;
};

__constant__ unsigned char RD_FONT[10][7] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},
    {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},
    {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},
    {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}};

__global__ __launch_bounds__(RD_THREADS) void render_digits_kernel(rd_digits_p p) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * RD_WAVES + ((int)threadIdx.x >> 6);
    const int m = (int)(w / p.t.V), v = (int)(w % p.t.V);
    if (m >= p.M) return;
    const int value = p.values[m];
    if (value < 0) return;
    float pu, pv;
    if (p.planar) {
        pu = p.anchors[(int64_t)m * 2], pv = p.anchors[(int64_t)m * 2 + 1];
    } else {
        const float x = p.anchors[(int64_t)m * 3], y = p.anchors[(int64_t)m * 3 + 1], z = p.anchors[(int64_t)m * 3 + 2];
        if (!(finite32(x) && finite32(y) && finite32(z))) return;
        const float r3 = rd_row(p.t, v, 3, x, y, z);
        if (!(r3 >= p.t.near)) return;
        const float r0 = rd_row(p.t, v, 0, x, y, z), r1 = rd_row(p.t, v, 1, x, y, z);
        pu = r0 / r3, pv = r1 / r3;
    }
    if (!(pu >= -65536.f && pu < 65536.f && pv >= -65536.f && pv < 65536.f)) return;
    const int X0 = (int)floorf(pu), Y0 = (int)floorf(pv);
    int nd = 1;
    for (int q = value / 10; q > 0; q /= 10) ++nd;
    int rank = p.rank ? p.rank[m] : m;
    if (rank < 0) rank = 0;
    const u64 key = rd_key(p.t.layer, 0xFFFFFFFFu - (unsigned)rank, p.rgb ? p.rgb[m] : p.rgb_one);
    for (int e = lane; e < nd * 35; e += 64) {
        const int j = e / 35, cell = e % 35, cy = cell / 5, cx = cell % 5;
        int q = value;
        for (int s = nd - 1 - j; s > 0; --s) q /= 10;
        const int g = q % 10;
        if (!((RD_FONT[g][cy] >> (4 - cx)) & 1)) continue;
        const int bx = X0 + (6 * j + cx) * p.scale, by = Y0 + cy * p.scale;
        for (int l = 0; l < p.scale; ++l)
            for (int i = 0; i < p.scale; ++i) rd_put(p.t, v, bx + i, by + l, key);
    }
}

// ---- cmt_render_resolve ----------------------------------------------------------------------------------------
struct rd_resolve_p {
    const u64* plane;
    const unsigned char* src;
    unsigned char* out;
    int64_t total;
    unsigned background;
};

__global__ __launch_bounds__(RD_THREADS) void render_resolve_kernel(rd_resolve_p p) {
    const int64_t i = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= p.total) return;
    const u64 key = p.plane[i];
    unsigned rgb = (unsigned)key & 0xFFFFFFu;
    if (key == 0ull) {
        rgb = p.background & 0xFFFFFFu;
        if (p.src) rgb = ((unsigned)p.src[3 * i] << 16) | ((unsigned)p.src[3 * i + 1] << 8) | (unsigned)p.src[3 * i + 2];
    }
    p.out[3 * i] = (unsigned char)(rgb >> 16);
    p.out[3 * i + 1] = (unsigned char)(rgb >> 8);
    p.out[3 * i + 2] = (unsigned char)rgb;
}

// ---- host ------------------------------------------------------------------------------------------------------
extern "C" int64_t cmt_render_points_args_size(void) { return (int64_t)sizeof(cmt_render_points_args); }
extern "C" int64_t cmt_render_segments_args_size(void) { return (int64_t)sizeof(cmt_render_segments_args); }
extern "C" int64_t cmt_render_boxes_args_size(void) { return (int64_t)sizeof(cmt_render_boxes_args); }
extern "C" int64_t cmt_render_digits_args_size(void) { return (int64_t)sizeof(cmt_render_digits_args); }
extern "C" int64_t cmt_render_resolve_args_size(void) { return (int64_t)sizeof(cmt_render_resolve_args); }

static inline bool rd_size_ok(int V, int H, int W) {
    return V >= 1 && V <= CMT_RENDER_MAX_VIEWS && H >= 1 && H <= CMT_RENDER_MAX_SIZE && W >= 1 && W <= CMT_RENDER_MAX_SIZE;
}

// the checks every drawing call shares; uses_view: the view matrices are read
static int rd_target_check(const cmt_render_target& a, bool uses_view, rd_target& t, const char* who) {
    const std::string w(who);
    if (!rd_size_ok(a.V, a.H, a.W)) return cmt_fail(CMT_EINVAL, w + ": V must be 1..8, H and W 1..4096");
    if (a.layer < 0 || a.layer > 255) return cmt_fail(CMT_EINVAL, w + ": layer must be 0..255");
    if (!std::isfinite(a.near)) return cmt_fail(CMT_EINVAL, w + ": near must be finite");
    if (!ptr_aligned(a.plane, 8)) return cmt_fail(CMT_EINVAL, w + ": plane must be non-null and 8-byte aligned");
    for (int v = 0; v < CMT_RENDER_MAX_VIEWS; ++v)
        for (int e = 0; e < 16; ++e) {
            const bool used = uses_view && v < a.V;
            if (used && !std::isfinite(a.view[v][e])) return cmt_fail(CMT_EINVAL, w + ": a view entry is not finite");
            t.view[v][e] = used ? a.view[v][e] : 0.f;
        }
    t.plane = (u64*)a.plane, t.V = a.V, t.H = a.H, t.W = a.W, t.layer = (unsigned)a.layer, t.near = a.near;
    return 0;
}

#define RD_TARGET(args, uses_view, dst, who)                              \
    do {                                                                  \
        const int rc_ = rd_target_check((args)->t, uses_view, dst, who);  \
        if (rc_ != 0) return rc_;                                         \
    } while (0)

extern "C" int cmt_render_points(const cmt_render_points_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_render_points: null argument struct");
    rd_points_p p;
    RD_TARGET(a, true, p.t, "cmt_render_points");
    CMT_REQUIRE(a->N >= 0, "cmt_render_points: N must be 0 .. 2^31 - 1");
    CMT_REQUIRE(a->ld >= 3, "cmt_render_points: ld must be at least 3");
    CMT_REQUIRE(a->color_col >= -1 && a->color_col < a->ld, "cmt_render_points: color_col must be -1 .. ld - 1");
    CMT_REQUIRE(a->radius >= 0 && a->radius <= 2, "cmt_render_points: radius must be 0..2");
    CMT_REQUIRE(std::isfinite(a->lo) && std::isfinite(a->inv_span), "cmt_render_points: lo and inv_span must be finite");
    CMT_REQUIRE(ptr_aligned_or_null(a->points, 4) && ptr_aligned_or_null(a->lut, 4) && ptr_aligned_or_null(a->n, 4),
                "cmt_render_points: points, lut and n must be 4-byte aligned");
    CMT_REQUIRE(a->N == 0 || (a->points != nullptr && a->lut != nullptr), "cmt_render_points: points and lut must be non-null with N > 0");
    if (a->N == 0) return 0;
    p.points = (const float*)a->points, p.n = a->n, p.lut = (const unsigned*)a->lut;
    p.N = a->N, p.ld = a->ld, p.radius = a->radius, p.near_wins = a->near_wins ? 1 : 0, p.color_col = a->color_col;
    p.lo = a->lo, p.inv_span = a->inv_span;
    int64_t blocks = cdiv64(a->N, RD_THREADS);
    const int64_t cap = (int64_t)cmt_cu_count() * 8;
    if (blocks > cap) blocks = cap;
    render_points_kernel<<<dim3((unsigned)blocks), RD_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_render_points");
}

static inline bool rd_items_ok(int n) { return n >= 0 && n < CMT_RENDER_MAX_ITEMS; }

extern "C" int cmt_render_segments(const cmt_render_segments_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_render_segments: null argument struct");
    rd_segments_p p;
    RD_TARGET(a, a->planar == 0, p.t, "cmt_render_segments");
    CMT_REQUIRE(rd_items_ok(a->S), "cmt_render_segments: S must be 0 .. 2^20 - 1");
    CMT_REQUIRE(a->thickness >= 1 && a->thickness <= 3, "cmt_render_segments: thickness must be 1..3");
    CMT_REQUIRE(ptr_aligned_or_null(a->p0, 4) && ptr_aligned_or_null(a->p1, 4) && ptr_aligned_or_null(a->rgb, 4) &&
                    ptr_aligned_or_null(a->rank, 4) && ptr_aligned_or_null(a->n, 4),
                "cmt_render_segments: p0, p1, rgb, rank and n must be 4-byte aligned");
    CMT_REQUIRE(a->S == 0 || (a->p0 != nullptr && a->p1 != nullptr && a->rgb != nullptr),
                "cmt_render_segments: p0, p1 and rgb must be non-null with S > 0");
    if (a->S == 0) return 0;
    p.p0 = (const float*)a->p0, p.p1 = (const float*)a->p1, p.rgb = (const unsigned*)a->rgb, p.rank = a->rank, p.n = a->n;
    p.S = a->S, p.planar = a->planar ? 1 : 0, p.thick = a->thickness;
    const int64_t blocks = cdiv64((int64_t)a->S * p.t.V, RD_WAVES);
    render_segments_kernel<<<dim3((unsigned)blocks), RD_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_render_segments");
}

extern "C" int cmt_render_boxes(const cmt_render_boxes_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_render_boxes: null argument struct");
    rd_boxes_p p;
    RD_TARGET(a, true, p.t, "cmt_render_boxes");
    CMT_REQUIRE(rd_items_ok(a->M), "cmt_render_boxes: M must be 0 .. 2^20 - 1");
    CMT_REQUIRE(a->ld >= 7, "cmt_render_boxes: ld must be at least 7");
    CMT_REQUIRE(a->z_origin == 0.f || a->z_origin == 0.5f, "cmt_render_boxes: z_origin must be 0 or 0.5");
    CMT_REQUIRE(a->thickness >= 1 && a->thickness <= 3, "cmt_render_boxes: thickness must be 1..3");
    CMT_REQUIRE(!std::isnan(a->score_thr), "cmt_render_boxes: score_thr must not be NaN");
    CMT_REQUIRE(a->ncls >= 0, "cmt_render_boxes: ncls must not be negative");
    CMT_REQUIRE(ptr_aligned_or_null(a->boxes, 4) && ptr_aligned_or_null(a->count, 4) && ptr_aligned_or_null(a->labels, 4) &&
                    ptr_aligned_or_null(a->scores, 4) && ptr_aligned_or_null(a->class_rgb, 4),
                "cmt_render_boxes: boxes, count, labels, scores and class_rgb must be 4-byte aligned");
    CMT_REQUIRE(a->M == 0 || a->boxes != nullptr, "cmt_render_boxes: boxes must be non-null with M > 0");
    if (a->M == 0) return 0;
    p.boxes = (const float*)a->boxes, p.count = a->count, p.labels = a->labels, p.scores = (const float*)a->scores;
    p.class_rgb = (const unsigned*)a->class_rgb;
    p.M = a->M, p.ld = a->ld, p.thick = a->thickness, p.ncls = a->ncls;
    p.z_origin = a->z_origin, p.score_thr = a->score_thr, p.rgb_default = a->rgb_default;
    const int64_t blocks = cdiv64((int64_t)a->M * p.t.V, RD_WAVES);
    render_boxes_kernel<<<dim3((unsigned)blocks), RD_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_render_boxes");
}

extern "C" int cmt_render_digits(const cmt_render_digits_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_render_digits: null argument struct");
    rd_digits_p p;
    RD_TARGET(a, a->planar == 0, p.t, "cmt_render_digits");
    CMT_REQUIRE(rd_items_ok(a->M), "cmt_render_digits: M must be 0 .. 2^20 - 1");
    CMT_REQUIRE(a->scale >= 1 && a->scale <= 4, "cmt_render_digits: scale must be 1..4");
    CMT_REQUIRE(ptr_aligned_or_null(a->values, 4) && ptr_aligned_or_null(a->anchors, 4) && ptr_aligned_or_null(a->rgb, 4) &&
                    ptr_aligned_or_null(a->rank, 4),
                "cmt_render_digits: values, anchors, rgb and rank must be 4-byte aligned");
    CMT_REQUIRE(a->M == 0 || (a->values != nullptr && a->anchors != nullptr), "cmt_render_digits: values and anchors must be non-null with M > 0");
    if (a->M == 0) return 0;
    p.values = (const int*)a->values, p.anchors = (const float*)a->anchors, p.rgb = (const unsigned*)a->rgb, p.rank = a->rank;
    p.M = a->M, p.planar = a->planar ? 1 : 0, p.scale = a->scale, p.rgb_one = a->rgb_one;
    const int64_t blocks = cdiv64((int64_t)a->M * p.t.V, RD_WAVES);
    render_digits_kernel<<<dim3((unsigned)blocks), RD_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_render_digits");
}

extern "C" int cmt_render_resolve(const cmt_render_resolve_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_render_resolve: null argument struct");
    CMT_REQUIRE(rd_size_ok(a->V, a->H, a->W), "cmt_render_resolve: V must be 1..8, H and W 1..4096");
    CMT_REQUIRE(ptr_aligned(a->plane, 8), "cmt_render_resolve: plane must be non-null and 8-byte aligned");
    CMT_REQUIRE(a->out != nullptr, "cmt_render_resolve: out must be non-null");
    rd_resolve_p p;
    p.plane = (const u64*)a->plane, p.src = (const unsigned char*)a->src, p.out = (unsigned char*)a->out;
    p.total = (int64_t)a->V * a->H * a->W, p.background = a->background;
    render_resolve_kernel<<<dim3((unsigned)cdiv64(p.total, RD_THREADS)), RD_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_render_resolve");
}
