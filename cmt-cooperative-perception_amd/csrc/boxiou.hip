// Rotated-box overlap of include/cmt_hip.h on the device:
//   cmt_box_iou:    the pairwise (or row-by-row) BEV and 3D IoU of two box sets;
//   cmt_box_nms:    greedy rotated NMS of one set: rank, suppression matrix, scan;
//   cmt_box_concat: the candidate set of late fusion, K sources with a rigid transform each.
//
// The overlap of one pair (the frame change, the clip in a per-lane LDS slot, the quotients) is box_overlap.h,
// shared with deteval.hip.  The pairwise kernel and the suppression-matrix kernel share one tile shape: 64 x 64 pairs, 256 threads, a lane
// owns a column and a wave walks 16 rows; the derived values of the tile's 64 + 64 boxes (one sinf / cosf pair
// each) are computed once per workgroup and staged in LDS.  In the matrix kernel the 64 lanes of a wave are the 64
// bits of one word: a ballot builds it and lane 0 stores it.
// No atomics and no workgroup waits for another: results are bitwise repeatable.
// The file is built with -ffp-contract=off: every product, sum and quotient of the contract is rounded on its own.
#include "box_overlap.h"
#include "box_rigid.h"
#include "wave_ops.h"

#include <cmath>

constexpr int BI_TILE = 64;
constexpr int BI_WROWS = 16;                 // rows of a tile one wave walks
constexpr int NMS_RANK_THREADS = 1024;
constexpr int NMS_AHEAD = 8;                 // mask rows the scan loads ahead of the row it decides
static_assert(CMT_NMS_MAX == 2 * NMS_RANK_THREADS, "the bitonic network does one exchange per thread and step at the cap");
static_assert(CMT_NMS_MAX / 64 <= 64, "a lane per word of the removed set");

typedef unsigned long long u64;

// ---- cmt_box_iou ---------------------------------------------------------------------------------------------
struct bi_p {
    const float* a;
    const float* b;
    const int* n_a;
    const int* n_b;
    float* bev;
    float* iou3d;
    int N, M, lda, ldb, tiles_x;
    int64_t ldo;
    float z_origin;
};

__global__ __launch_bounds__(BI_THREADS) void box_iou_kernel(bi_p p) {
    __shared__ float px[2 * BI_SLOT], py[2 * BI_SLOT];
    __shared__ bi_box sa[BI_TILE], sb[BI_TILE];
    const int na = clamp_count(p.n_a, p.N), nb = clamp_count(p.n_b, p.M);
    const int tile = (int)blockIdx.x;
    const int r0 = (tile / p.tiles_x) * BI_TILE, c0 = (tile % p.tiles_x) * BI_TILE;
    if (r0 >= na || c0 >= nb) return;
    const int tid = (int)threadIdx.x;
    if (tid < BI_TILE) {
        const int j = c0 + tid;
        sb[tid] = j < nb ? bi_derive(p.b + (int64_t)j * p.ldb, p.z_origin) : bi_none();
    } else if (tid < 2 * BI_TILE) {
        const int i = r0 + tid - BI_TILE;
        sa[tid - BI_TILE] = i < na ? bi_derive(p.a + (int64_t)i * p.lda, p.z_origin) : bi_none();
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    const int j = c0 + lane;
    if (j >= nb) return;   // after the only barrier
    const bi_box B = sb[lane];
    for (int k = 0; k < BI_WROWS; ++k) {
        const int i = r0 + w * BI_WROWS + k;
        if (i >= na) break;
        const bi_box A = sa[w * BI_WROWS + k];
        float bev = 0.f, v3 = 0.f;
        if (A.ok && B.ok) {
            float area, h;
            bi_pair(A, B, px + tid, py + tid, area, h);
            bev = bi_bev(A, B, area);
            v3 = bi_3d(A, B, area, h);
        }
        const int64_t o = (int64_t)i * p.ldo + j;
        if (p.bev) p.bev[o] = bev;
        if (p.iou3d) p.iou3d[o] = v3;
    }
}

__global__ __launch_bounds__(BI_THREADS) void box_iou_aligned_kernel(bi_p p) {
    __shared__ float px[2 * BI_SLOT], py[2 * BI_SLOT];
    const int na = clamp_count(p.n_a, p.N), nb = clamp_count(p.n_b, p.M);
    const int n = na < nb ? na : nb;
    const int tid = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BI_THREADS + tid;
    if (i >= n) return;
    const bi_box A = bi_derive(p.a + i * p.lda, p.z_origin), B = bi_derive(p.b + i * p.ldb, p.z_origin);
    float bev = 0.f, v3 = 0.f;
    if (A.ok && B.ok) {
        float area, h;
        bi_pair(A, B, px + tid, py + tid, area, h);
        bev = bi_bev(A, B, area);
        v3 = bi_3d(A, B, area, h);
    }
    if (p.bev) p.bev[i] = bev;
    if (p.iou3d) p.iou3d[i] = v3;
}

// ---- cmt_box_nms ---------------------------------------------------------------------------------------------
// workspace: int32 n_valid, 3 words of padding, order int32 [Np], mask uint64 [Np][W]; Np = N rounded up to 64,
// W = Np / 64.
struct nms_p {
    const float* boxes;
    const float* scores;
    const int* labels;
    const int* count;
    int* nv;
    int* order;
    u64* mask;
    int* keep_idx;
    void* keep;
    int* keep_count;
    int N, ld, P, W, use_3d, keep_i32;
    float iou_thr, score_thr, z_origin;
};

__device__ __forceinline__ unsigned nms_hi(u64 k) { return (unsigned)(k >> 32); }

__global__ __launch_bounds__(NMS_RANK_THREADS) void nms_rank_kernel(nms_p p) {
    __shared__ u64 key[CMT_NMS_MAX];
    const int tid = (int)threadIdx.x;
    const int n = clamp_count(p.count, p.N);
    for (int e = tid; e < p.P; e += NMS_RANK_THREADS) {
        unsigned hi = 0xFFFFFFFFu;
        if (e < n) {
            const float s = p.scores[e];
            if (s >= p.score_thr) hi = score_desc_key(s);   // false for a NaN score; at most 0xFF800000 (-inf), never all ones
        }
        key[e] = ((u64)hi << 32) | (unsigned)e;
    }
    for (int k = 2; k <= p.P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < (p.P >> 1); t += NMS_RANK_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const bool up = (i & k) == 0;
                const u64 a = key[i], b = key[l];
                if ((a > b) == up) key[i] = b, key[l] = a;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < p.N; e += NMS_RANK_THREADS) {
        p.order[e] = (int)(unsigned)key[e];
        const bool v = nms_hi(key[e]) != 0xFFFFFFFFu;
        const bool vn = e + 1 < p.N && nms_hi(key[e + 1]) != 0xFFFFFFFFu;
        if (v && !vn) *p.nv = e + 1;          // one writer: the last existing rank
    }
    if (tid == 0 && (p.N == 0 || nms_hi(key[0]) == 0xFFFFFFFFu)) *p.nv = 0;
}

__global__ __launch_bounds__(BI_THREADS) void nms_mask_kernel(nms_p p) {
    __shared__ float px[2 * BI_SLOT], py[2 * BI_SLOT];
    __shared__ bi_box sa[BI_TILE], sb[BI_TILE];
    __shared__ int la[BI_TILE], lb[BI_TILE];
    const int nv = clamp_count(p.nv, p.N);
    const int wv = (nv + 63) >> 6;
    const int ti = (int)blockIdx.x / p.W, tj = (int)blockIdx.x % p.W;
    if (tj < ti || tj >= wv) return;          // the upper triangle of the existing ranks
    const int tid = (int)threadIdx.x;
    if (tid < 2 * BI_TILE) {
        const bool col = tid < BI_TILE;
        const int e = col ? tid : tid - BI_TILE;
        const int r = (col ? tj : ti) * BI_TILE + e;
        bi_box d = bi_none();
        int lab = 0;
        if (r < nv) {
            const int row = clamp_index(p.order[r], p.N - 1);
            d = bi_derive(p.boxes + (int64_t)row * p.ld, p.z_origin);
            if (p.labels) lab = p.labels[row];
        }
        if (col) sb[e] = d, lb[e] = lab;
        else sa[e] = d, la[e] = lab;
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    const int c = tj * BI_TILE + lane;
    const bi_box B = sb[lane];
    const int labB = lb[lane];
    for (int k = 0; k < BI_WROWS; ++k) {
        const int r = ti * BI_TILE + w * BI_WROWS + k;
        if (r >= nv) break;
        const bi_box A = sa[w * BI_WROWS + k];
        bool sup = false;
        if (c < nv && c > r && A.ok && B.ok && la[w * BI_WROWS + k] == labB) {
            float area, h;
            bi_pair(A, B, px + tid, py + tid, area, h);
            const float v = p.use_3d ? bi_3d(A, B, area, h) : bi_bev(A, B, area);
            sup = v > p.iou_thr;
        }
        const u64 word = __ballot(sup);
        if (lane == 0) p.mask[(int64_t)r * p.W + tj] = word;
    }
}

__device__ __forceinline__ u64 nms_readlane(u64 v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void nms_scan_kernel(nms_p p) {
    const int lane = (int)threadIdx.x;
    const int nv = __builtin_amdgcn_readfirstlane(clamp_count(p.nv, p.N));
    const int wv = (nv + 63) >> 6;
    // word `lane` of mask row r; words left of the diagonal tile and rows at or beyond nv were never written
    auto load = [&](int r) -> u64 {
        return (r < nv && lane >= (r >> 6) && lane < wv) ? p.mask[(int64_t)r * p.W + lane] : 0ull;
    };
    u64 removed = 0ull, cur[NMS_AHEAD], nxt[NMS_AHEAD];
#pragma unroll
    for (int k = 0; k < NMS_AHEAD; ++k) cur[k] = load(k);
    for (int r0 = 0; r0 < nv; r0 += NMS_AHEAD) {
#pragma unroll
        for (int k = 0; k < NMS_AHEAD; ++k) nxt[k] = load(r0 + NMS_AHEAD + k);   // they do not depend on the outcome
#pragma unroll
        for (int k = 0; k < NMS_AHEAD; ++k) {
            const int r = r0 + k;
            if (r < nv) {
                const u64 wd = nms_readlane(removed, r >> 6);
                if (!((wd >> (r & 63)) & 1ull)) removed |= cur[k];
            }
        }
#pragma unroll
        for (int k = 0; k < NMS_AHEAD; ++k) cur[k] = nxt[k];
    }
    // a bit of `removed` is only ever set for a rank after the row that sets it: kept = existing and not removed
    u64 valid = 0ull;
    if (lane < wv) valid = (lane == wv - 1 && (nv & 63)) ? ((1ull << (nv & 63)) - 1ull) : ~0ull;
    const u64 kw = ~removed & valid;
    int base = 0;
    for (int w = 0; w < p.W; ++w) {
        const u64 k = w < wv ? nms_readlane(kw, w) : 0ull;
        const int r = w * 64 + lane;
        const bool bit = (k >> lane) & 1ull;
        if (r < p.N) {
            const int row = clamp_index(p.order[r], p.N - 1);
            if (bit) p.keep_idx[base + __popcll(k & ((1ull << lane) - 1ull))] = row;
            if (p.keep) {
                if (p.keep_i32) ((int*)p.keep)[row] = bit ? 1 : 0;
                else ((unsigned char*)p.keep)[row] = bit ? 1 : 0;
            }
        }
        base += __popcll(k);
    }
    for (int e = base + lane; e < p.N; e += 64) p.keep_idx[e] = -1;
    if (lane == 0) *p.keep_count = base;
}

// ---- cmt_box_concat ------------------------------------------------------------------------------------------
struct bc_p {
    const float* boxes[CMT_CONCAT_MAX];
    const float* scores[CMT_CONCAT_MAX];
    const int* labels[CMT_CONCAT_MAX];
    const int* count[CMT_CONCAT_MAX];
    int n[CMT_CONCAT_MAX], ld[CMT_CONCAT_MAX], has_tf[CMT_CONCAT_MAX];
    float m[CMT_CONCAT_MAX][12];
    float yaw[CMT_CONCAT_MAX];
    float* ob;
    float* os;
    int* ol;
    int* osrc;
    int* ocount;
    int K, cols, ld_out, total;
};

__global__ __launch_bounds__(256) void box_concat_kernel(bc_p p) {
#pragma clang fp contract(off)
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e == 0) *p.ocount = p.total;
    if (e >= p.total) return;
    // the source of row e: statically indexed selects over the (at most 8) segments
    const float* src = nullptr;
    const float* sc = nullptr;
    const int* lb = nullptr;
    const int* cnt = nullptr;
    int k = 0, i = 0, nk = 0, ld = 0, has = 0, off = 0;
    float m[12], yaw = 0.f;
#pragma unroll
    for (int t = 0; t < 12; ++t) m[t] = 0.f;
#pragma unroll
    for (int q = 0; q < CMT_CONCAT_MAX; ++q) {
        if (q < p.K) {
            if (e >= off && e < off + p.n[q]) {
                src = p.boxes[q], sc = p.scores[q], lb = p.labels[q], cnt = p.count[q];
                k = q, i = e - off, nk = p.n[q], ld = p.ld[q], has = p.has_tf[q], yaw = p.yaw[q];
#pragma unroll
                for (int t = 0; t < 12; ++t) m[t] = p.m[q][t];
            }
            off += p.n[q];
        }
    }
    const int c = clamp_count(cnt, nk);
    float* o = p.ob + (int64_t)e * p.ld_out;
    p.osrc[e] = k;
    if (i >= c) {
        for (int t = 0; t < p.cols; ++t) o[t] = 0.f;
        p.os[e] = -__builtin_inff();
        p.ol[e] = -1;
        return;
    }
    const float* r = src + (int64_t)i * ld;
    p.os[e] = sc[i];
    p.ol[e] = lb[i];
    if (!has) {
        for (int t = 0; t < p.cols; ++t) o[t] = r[t];
        return;
    }
    const bool has_vel = p.cols >= 9;   // below 9 columns box_rigid's velocity runs on zeros and is dropped (r[7], r[8] may not exist)
    float pos[3], vel[2];
    box_rigid(m, r[0], r[1], r[2], has_vel ? r[7] : 0.f, has_vel ? r[8] : 0.f, pos, vel);
    o[0] = pos[0], o[1] = pos[1], o[2] = pos[2];
    o[3] = r[3], o[4] = r[4], o[5] = r[5];
    o[6] = r[6] + yaw;
    if (has_vel) {
        o[7] = vel[0], o[8] = vel[1];
        for (int t = 9; t < p.cols; ++t) o[t] = r[t];
    } else {
        for (int t = 7; t < p.cols; ++t) o[t] = r[t];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------
extern "C" int64_t cmt_box_iou_args_size(void) { return (int64_t)sizeof(cmt_box_iou_args); }
extern "C" int64_t cmt_box_nms_args_size(void) { return (int64_t)sizeof(cmt_box_nms_args); }
extern "C" int64_t cmt_box_concat_args_size(void) { return (int64_t)sizeof(cmt_box_concat_args); }

static inline bool bi_zo(float z) { return z == 0.f || z == 0.5f; }

extern "C" int64_t cmt_box_nms_workspace_bytes(int N) {
    if (N < 0 || N > CMT_NMS_MAX) return -1;
    const int64_t np = cdiv64(N, 64) * 64;
    return 16 + 4 * np + 8 * np * (np / 64);
}

extern "C" int cmt_box_iou(const cmt_box_iou_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_box_iou: null argument struct");
    CMT_REQUIRE(a->N >= 0 && a->M >= 0, "cmt_box_iou: N and M must not be negative");
    CMT_REQUIRE(a->lda >= 7 && a->ldb >= 7, "cmt_box_iou: lda and ldb must be at least 7");
    CMT_REQUIRE(bi_zo(a->z_origin), "cmt_box_iou: z_origin must be 0 or 0.5");
    CMT_REQUIRE(a->bev != nullptr || a->iou3d != nullptr, "cmt_box_iou: bev and iou3d must not both be null");
    CMT_REQUIRE(!a->aligned || a->N == a->M, "cmt_box_iou: aligned needs N == M");
    CMT_REQUIRE(a->aligned || a->ldo >= a->M, "cmt_box_iou: ldo must be at least M");
    CMT_REQUIRE(cdiv64(a->N, BI_TILE) * cdiv64(a->M, BI_TILE) < (int64_t)1 << 31, "cmt_box_iou: N * M / 4096 must stay below 2^31 tiles");
    CMT_REQUIRE(ptr_aligned_or_null(a->bev, 4) && ptr_aligned_or_null(a->iou3d, 4), "cmt_box_iou: bev and iou3d must be 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->n_a, 4) && ptr_aligned_or_null(a->n_b, 4), "cmt_box_iou: n_a and n_b must be 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->a, 4) && ptr_aligned_or_null(a->b, 4) && (a->N == 0 || a->M == 0 || (a->a != nullptr && a->b != nullptr)),
                "cmt_box_iou: a and b must be non-null (with N, M > 0) and 4-byte aligned");
    if (a->N == 0 || a->M == 0) return 0;
    bi_p p;
    p.a = (const float*)a->a, p.b = (const float*)a->b, p.n_a = a->n_a, p.n_b = a->n_b;
    p.bev = (float*)a->bev, p.iou3d = (float*)a->iou3d;
    p.N = a->N, p.M = a->M, p.lda = a->lda, p.ldb = a->ldb, p.ldo = a->ldo, p.z_origin = a->z_origin;
    p.tiles_x = (int)cdiv64(a->M, BI_TILE);
    const hipStream_t st = (hipStream_t)stream;
    if (a->aligned) {
        box_iou_aligned_kernel<<<dim3((unsigned)cdiv64(a->N, BI_THREADS)), BI_THREADS, 0, st>>>(p);
    } else {
        box_iou_kernel<<<dim3((unsigned)(cdiv64(a->N, BI_TILE) * p.tiles_x)), BI_THREADS, 0, st>>>(p);
    }
    return cmt_check_launch("cmt_box_iou");
}

extern "C" int cmt_box_nms(const cmt_box_nms_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_box_nms: null argument struct");
    CMT_REQUIRE(a->N >= 0 && a->N <= CMT_NMS_MAX, "cmt_box_nms: N must be 0..2048");
    CMT_REQUIRE(a->ld >= 7, "cmt_box_nms: ld must be at least 7");
    CMT_REQUIRE(bi_zo(a->z_origin), "cmt_box_nms: z_origin must be 0 or 0.5");
    CMT_REQUIRE(std::isfinite(a->iou_thr) && a->iou_thr >= 0.f, "cmt_box_nms: iou_thr must be finite and not negative");
    CMT_REQUIRE(!std::isnan(a->score_thr), "cmt_box_nms: score_thr must not be NaN");
    CMT_REQUIRE(a->keep_dtype == 0 || a->keep_dtype == 1, "cmt_box_nms: keep_dtype must be 0 (uint8) or 1 (int32)");
    CMT_REQUIRE(a->N == 0 || (ptr_aligned(a->boxes, 4) && ptr_aligned(a->scores, 4)), "cmt_box_nms: boxes and scores must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->labels, 4) && ptr_aligned_or_null(a->count, 4), "cmt_box_nms: labels and count must be 4-byte aligned");
    CMT_REQUIRE(a->N == 0 || ptr_aligned(a->keep_idx, 4), "cmt_box_nms: keep_idx must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->keep, a->keep_dtype ? 4 : 1), "cmt_box_nms: an int32 keep must be 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->keep_count, 4), "cmt_box_nms: keep_count must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->workspace, 8), "cmt_box_nms: workspace must be non-null and 8-byte aligned");
    CMT_REQUIRE(a->workspace_bytes >= cmt_box_nms_workspace_bytes(a->N), "cmt_box_nms: workspace_bytes is below cmt_box_nms_workspace_bytes(N)");
    const int np = (int)cdiv64(a->N, 64) * 64;
    nms_p p;
    p.boxes = (const float*)a->boxes, p.scores = (const float*)a->scores, p.labels = a->labels, p.count = a->count;
    p.nv = (int*)a->workspace;
    p.order = p.nv + 4;
    p.mask = (u64*)(p.order + np);
    p.keep_idx = a->keep_idx, p.keep = a->keep, p.keep_count = a->keep_count;
    p.N = a->N, p.ld = a->ld, p.W = np / 64, p.use_3d = a->use_3d ? 1 : 0, p.keep_i32 = a->keep_dtype;
    p.P = 2;
    while (p.P < a->N) p.P <<= 1;
    p.iou_thr = a->iou_thr, p.score_thr = a->score_thr, p.z_origin = a->z_origin;
    const hipStream_t st = (hipStream_t)stream;
    nms_rank_kernel<<<dim3(1), NMS_RANK_THREADS, 0, st>>>(p);
    if (p.W > 0) nms_mask_kernel<<<dim3((unsigned)(p.W * p.W)), BI_THREADS, 0, st>>>(p);
    nms_scan_kernel<<<dim3(1), 64, 0, st>>>(p);
    return cmt_check_launch("cmt_box_nms");
}

extern "C" int cmt_box_concat(const cmt_box_concat_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_box_concat: null argument struct");
    CMT_REQUIRE(a->K >= 1 && a->K <= CMT_CONCAT_MAX, "cmt_box_concat: K must be 1..8");
    CMT_REQUIRE(a->cols >= 7 && a->cols <= 16, "cmt_box_concat: cols must be 7..16");
    CMT_REQUIRE(a->ld_out >= a->cols, "cmt_box_concat: ld_out must be at least cols");
    int64_t total = 0;
    bc_p p;
    for (int k = 0; k < CMT_CONCAT_MAX; ++k) {
        p.boxes[k] = nullptr, p.scores[k] = nullptr, p.labels[k] = nullptr, p.count[k] = nullptr;
        p.n[k] = 0, p.ld[k] = 0, p.has_tf[k] = 0, p.yaw[k] = 0.f;
        for (int t = 0; t < 12; ++t) p.m[k][t] = 0.f;
    }
    for (int k = 0; k < a->K; ++k) {
        CMT_REQUIRE(a->n[k] >= 0, "cmt_box_concat: a source's capacity must not be negative");
        CMT_REQUIRE(a->ld[k] >= a->cols, "cmt_box_concat: a source's ld must be at least cols");
        CMT_REQUIRE(a->n[k] == 0 || (ptr_aligned(a->boxes[k], 4) && ptr_aligned(a->scores[k], 4) && ptr_aligned(a->labels[k], 4)),
                    "cmt_box_concat: a source's boxes, scores and labels must be non-null and 4-byte aligned");
        CMT_REQUIRE(ptr_aligned_or_null(a->count[k], 4), "cmt_box_concat: a source's count must be 4-byte aligned");
        if (a->has_transform[k]) {
            bool fin = true;
            for (int t = 0; t < 12; ++t) fin = fin && std::isfinite(a->transform[k][t]);
            CMT_REQUIRE(fin, "cmt_box_concat: a transform must be finite");
            p.yaw[k] = atan2f(a->transform[k][4], a->transform[k][0]);
            for (int t = 0; t < 12; ++t) p.m[k][t] = a->transform[k][t];
        }
        p.boxes[k] = (const float*)a->boxes[k], p.scores[k] = (const float*)a->scores[k];
        p.labels[k] = a->labels[k], p.count[k] = a->count[k];
        p.n[k] = a->n[k], p.ld[k] = a->ld[k], p.has_tf[k] = a->has_transform[k] ? 1 : 0;
        total += a->n[k];
    }
    CMT_REQUIRE(total < (int64_t)1 << 30, "cmt_box_concat: the total capacity must stay below 2^30");
    CMT_REQUIRE(total == 0 || (ptr_aligned(a->out_boxes, 4) && ptr_aligned(a->out_scores, 4) && ptr_aligned(a->out_labels, 4) && ptr_aligned(a->out_source, 4)),
                "cmt_box_concat: out_boxes, out_scores, out_labels and out_source must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->out_count, 4), "cmt_box_concat: out_count must be non-null and 4-byte aligned");
    p.ob = (float*)a->out_boxes, p.os = (float*)a->out_scores, p.ol = a->out_labels, p.osrc = a->out_source;
    p.ocount = a->out_count;
    p.K = a->K, p.cols = a->cols, p.ld_out = a->ld_out, p.total = (int)total;
    const unsigned blocks = (unsigned)(total > 0 ? cdiv64(total, 256) : 1);
    box_concat_kernel<<<dim3(blocks), 256, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_box_concat");
}
