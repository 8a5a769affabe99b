// The ground-truth database of include/cmt_hip.h on the device:
//   cmt_gtdb_extract: the points of every box of one frame as a segment (create_groundtruth_database's
//                     points[point_indices[:, i]] with the box's bottom centre subtracted);
//   cmt_gtdb_gather:  the paste rows of K chosen segments, each translated to its box centre, in one launch;
//   cmt_gtdb_collide: sample_class_v2's BEV collision test and greedy loop for all classes of one sample_all,
//                     in one workgroup.
//
// cmt_gtdb_extract has three launches and no workgroup waits for another.  gtdb_count_kernel owns a tile of AUG_T
// consecutive points (the slot layout of ptsaug.hip: slot c * 64 + lane of chunk c = r * 4 + wave) and stores the
// hits of every (tile, box) pair in the workspace, the boxes staged PIB_CB at a time.  gtdb_scan_kernel, one
// workgroup, sums them per box, scans the boxes into offsets[] and leaves for every pair the destination row of its
// first hit.  gtdb_scatter_kernel evaluates the same function on the same staged values again, ranks the hits of a
// box inside its tile (ballot / mbcnt inside a chunk, an LDS table over the chunks) and writes the rows.  A
// (tile, box chunk) pair without a hit is skipped: one wave loads the chunk's counts and a ballot of "count > 0"
// is the set of boxes the tile visits.  No atomics anywhere: the results are bitwise repeatable.
// cmt_gtdb_collide keeps the corners, the stand-up rectangles and a bit matrix (candidate rows x all boxes) in
// LDS; every matrix word has one writer; one wave runs the greedy loop with the live set in its lanes.
#include "aug_inside.h"

constexpr int GT_MAXC = CMT_GTDB_MAX_COLLIDE;
constexpr int GT_WORDS = GT_MAXC / 32;

// ---- cmt_gtdb_extract ---------------------------------------------------------------------------------------
struct gtx_p {
    const float* pts;
    const int* count_in;
    const float* boxes;
    float* rows;
    int* offsets;
    int* cnt;     // workspace [tiles][M]: hits of the pair
    int* base;    // workspace [tiles][M]: destination row of the pair's first hit
    long long cap;
    unsigned N;
    int M, F, D, tiles;
};

__device__ __forceinline__ void gtx_load(const gtx_p& p, int w, int lane, float (&x)[AUG_R], float (&y)[AUG_R],
                                         float (&z)[AUG_R]) {
    const unsigned t0 = blockIdx.x * (unsigned)AUG_T;
    const unsigned cnt = (unsigned)clamp_count(p.count_in, p.N);
#pragma unroll
    for (int r = 0; r < AUG_R; ++r) {
        const unsigned i = t0 + (unsigned)((r * 4 + w) * 64 + lane);
        x[r] = y[r] = z[r] = __builtin_nanf("");   // a row that does not exist is inside nothing
        if (i < cnt) {
            const float* q = p.pts + (int64_t)i * p.F;
            x[r] = q[0], y[r] = q[1], z[r] = q[2];
        }
    }
}

__global__ __launch_bounds__(AUG_THREADS) void gtdb_count_kernel(gtx_p p) {
    __shared__ aug_box bx[PIB_CB];
    __shared__ int wh[AUG_THREADS / 64][PIB_CB];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float x[AUG_R], y[AUG_R], z[AUG_R];
    gtx_load(p, w, lane, x, y, z);
    int* out = p.cnt + (int64_t)blockIdx.x * p.M;
    for (int b0 = 0; b0 < p.M; b0 += PIB_CB) {
        const int nb = p.M - b0 < PIB_CB ? p.M - b0 : PIB_CB;
        __syncthreads();   // the previous chunk has been read
        if ((int)threadIdx.x < nb) bx[threadIdx.x] = aug_stage(p.boxes + (int64_t)(b0 + (int)threadIdx.x) * p.D);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const aug_box box = bx[b];
            int hits = 0;
#pragma unroll
            for (int r = 0; r < AUG_R; ++r) hits += __popcll(__ballot(aug_inside(box, x[r], y[r], z[r])));
            if (lane == 0) wh[w][b] = hits;
        }
        __syncthreads();
        if ((int)threadIdx.x < nb) out[b0 + threadIdx.x] = wh[0][threadIdx.x] + wh[1][threadIdx.x] + wh[2][threadIdx.x] + wh[3][threadIdx.x];
    }
}

// one workgroup: thread t sums and later prefixes the columns t, t + 256, ... (coalesced); the scan over the boxes
// runs on four consecutive boxes per thread
__global__ __launch_bounds__(AUG_THREADS) void gtdb_scan_kernel(gtx_p p) {
    __shared__ int s[CMT_GTDB_MAX_BOXES];
    __shared__ int wt[AUG_THREADS / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int b = tid; b < CMT_GTDB_MAX_BOXES; b += AUG_THREADS) {
        int tot = 0;
        if (b < p.M)
            for (int t = 0; t < p.tiles; ++t) tot += p.cnt[(int64_t)t * p.M + b];
        s[b] = tot;
    }
    __syncthreads();
    int a[4], local = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = s[4 * tid + q], local += a[q];
    const int incl = wave_scan_incl(local);
    if (lane == 63) wt[w] = incl;
    __syncthreads();   // s has been read by every thread, wt is written
    int run = incl - local;
#pragma unroll
    for (int v = 0; v < AUG_THREADS / 64; ++v) run += v < w ? wt[v] : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = 4 * tid + q;
        s[b] = run;
        if (b <= p.M) p.offsets[b] = run;   // b == M: the total (boxes at and beyond M hold no hits)
        run += a[q];
    }
    if (tid == AUG_THREADS - 1 && p.M == CMT_GTDB_MAX_BOXES) p.offsets[p.M] = run;
    __syncthreads();
    for (int b = tid; b < p.M; b += AUG_THREADS) {
        int at = s[b];
        for (int t = 0; t < p.tiles; ++t) {
            const int64_t k = (int64_t)t * p.M + b;
            p.base[k] = at;
            at += p.cnt[k];
        }
    }
}

// Not on tile_rank (wave_ops.h): the chunk table is per box (cc[b]), one barrier covers the tables of all the boxes a
// tile visits and a chunk without a hit skips its walk; tile_rank would cost a barrier pair per box.
__global__ __launch_bounds__(AUG_THREADS) void gtdb_scatter_kernel(gtx_p p) {
    __shared__ aug_box bx[PIB_CB];
    __shared__ int cc[PIB_CB][AUG_CHUNKS];
    __shared__ int sbase[PIB_CB];
    __shared__ unsigned smask[2];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float x[AUG_R], y[AUG_R], z[AUG_R];
    gtx_load(p, w, lane, x, y, z);
    const unsigned t0 = blockIdx.x * (unsigned)AUG_T;
    const int64_t row0 = (int64_t)blockIdx.x * p.M;
    for (int b0 = 0; b0 < p.M; b0 += PIB_CB) {
        const int nb = p.M - b0 < PIB_CB ? p.M - b0 : PIB_CB;
        __syncthreads();   // the previous chunk's tables have been read
        if (w == 0) {
            const int c = lane < nb ? p.cnt[row0 + b0 + lane] : 0;
            const unsigned long long m = __ballot(c > 0);
            if (lane == 0) smask[0] = (unsigned)m, smask[1] = (unsigned)(m >> 32);
            if (lane < nb) sbase[lane] = p.base[row0 + b0 + lane];
        }
        __syncthreads();
        const unsigned long long mask = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)smask[0]) |
                                        ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)smask[1]) << 32);
        if (mask == 0) continue;   // no point of this tile is inside a box of this chunk (the same in every thread)
        if ((int)threadIdx.x < nb && ((mask >> threadIdx.x) & 1))
            bx[threadIdx.x] = aug_stage(p.boxes + (int64_t)(b0 + (int)threadIdx.x) * p.D);
        __syncthreads();
        for (unsigned long long mm = mask; mm; mm &= mm - 1) {
            const int b = __builtin_ctzll(mm);
            const aug_box box = bx[b];
#pragma unroll
            for (int r = 0; r < AUG_R; ++r) {
                const int hits = __popcll(__ballot(aug_inside(box, x[r], y[r], z[r])));
                if (lane == 0) cc[b][r * 4 + w] = hits;
            }
        }
        __syncthreads();
        for (unsigned long long mm = mask; mm; mm &= mm - 1) {
            const int b = __builtin_ctzll(mm);
            const aug_box box = bx[b];
#pragma unroll
            for (int r = 0; r < AUG_R; ++r) {
                const bool in = aug_inside(box, x[r], y[r], z[r]);
                const unsigned long long m = __ballot(in);
                if (m == 0) continue;
                const int c = r * 4 + w;
                int at = sbase[b];
                for (int v = 0; v < c; ++v) at += cc[b][v];
                const long long g = (long long)at + wave_rank(m);
                if (in && g < p.cap) {
#pragma clang fp contract(off)
                    const unsigned i = t0 + (unsigned)(c * 64 + lane);   // below *count_in <= N: the row exists
                    const float* src = p.pts + (int64_t)i * p.F;
                    float* q = p.rows + g * p.F;
                    q[0] = x[r] - box.cx, q[1] = y[r] - box.cy, q[2] = z[r] - box.zb;
                    for (int k = 3; k < p.F; ++k) ((unsigned*)q)[k] = ((const unsigned*)src)[k];
                }
            }
        }
    }
}

// ---- cmt_gtdb_gather ----------------------------------------------------------------------------------------
struct gtg_p {
    const float* rows;
    const int* seg_offset;
    const int* seg_len;
    const int* dst_offset;
    const float* centre;
    float* dst;
    long long n_rows, n_dst;
    int F;
};

__global__ __launch_bounds__(AUG_THREADS) void gtdb_gather_kernel(gtg_p p) {
#pragma clang fp contract(off)
    const int k = (int)blockIdx.y;
    const long long so = p.seg_offset[k], d0 = p.dst_offset[k];
    const int len = p.seg_len[k];
    const float cx = p.centre[3 * k], cy = p.centre[3 * k + 1], cz = p.centre[3 * k + 2];
    for (long long i = blockIdx.x * AUG_THREADS + threadIdx.x; i < len; i += gridDim.x * AUG_THREADS) {
        const long long s = so + i, d = d0 + i;
        if (s < 0 || s >= p.n_rows || d < 0 || d >= p.n_dst) continue;   // a table entry outside its buffer moves nothing
        const float* src = p.rows + s * p.F;
        float* q = p.dst + d * p.F;
        q[0] = src[0] + cx, q[1] = src[1] + cy, q[2] = src[2] + cz;
        for (int c = 3; c < p.F; ++c) ((unsigned*)q)[c] = ((const unsigned*)src)[c];
    }
}

// ---- cmt_gtdb_collide ---------------------------------------------------------------------------------------
struct gtc_p {
    const float* boxes;
    int* keep;
    int* count;
    int n_gt, n_s, D;
    unsigned first[GT_WORDS];   // bit i: candidate i is the first of its group
};

// every corner of Q strictly inside P: cross < 0 for each of P's edges, in the reference's loop order
__device__ __forceinline__ bool gtc_contains(const float* P, const float* Q) {
#pragma clang fp contract(off)
    for (int l = 0; l < 4; ++l) {
        const float qx = Q[2 * l], qy = Q[2 * l + 1];
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const float vx = P[2 * k1] - P[2 * k], vy = P[2 * k1 + 1] - P[2 * k + 1];
            const float m0 = vy * (P[2 * k] - qx), m1 = vx * (P[2 * k + 1] - qy);
            const float cross = m0 - m1;
            if (cross >= 0.f) return false;
        }
    }
    return true;
}

__device__ __forceinline__ bool gtc_collide(const float* P, const float* Q, const float* sp, const float* sq) {
#pragma clang fp contract(off)
    const float iw = fminf(sp[2], sq[2]) - fmaxf(sp[0], sq[0]);
    if (!(iw > 0.f)) return false;
    const float ih = fminf(sp[3], sq[3]) - fmaxf(sp[1], sq[1]);
    if (!(ih > 0.f)) return false;
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const float ax = P[2 * k], ay = P[2 * k + 1], bx = P[2 * k1], by = P[2 * k1 + 1];
        for (int l = 0; l < 4; ++l) {
            const int l1 = (l + 1) & 3;
            const float cx = Q[2 * l], cy = Q[2 * l + 1], dx = Q[2 * l1], dy = Q[2 * l1 + 1];
            const bool acd = (dy - ay) * (cx - ax) > (cy - ay) * (dx - ax);
            const bool bcd = (dy - by) * (cx - bx) > (cy - by) * (dx - bx);
            if (acd != bcd) {
                const bool abc = (cy - ay) * (bx - ax) > (by - ay) * (cx - ax);
                const bool abd = (dy - ay) * (bx - ax) > (by - ay) * (dx - ax);
                if (abc != abd) return true;
            }
        }
    }
    if (gtc_contains(P, Q)) return true;
    return gtc_contains(Q, P);
}

__device__ __forceinline__ unsigned gtc_range_bits(int a, int b, int word) {   // bits [a, b) that fall in the word
    const int lo = a > word * 32 ? a : word * 32;
    const int hi = b < word * 32 + 32 ? b : word * 32 + 32;
    if (hi <= lo) return 0u;
    const unsigned ones = hi - lo == 32 ? 0xffffffffu : ((1u << (hi - lo)) - 1u);
    return ones << (lo - word * 32);
}

__global__ __launch_bounds__(AUG_THREADS) void gtdb_collide_kernel(gtc_p p) {
    __shared__ float cor[GT_MAXC][8];
    __shared__ float su[GT_MAXC][4];
    __shared__ unsigned mat[GT_MAXC * GT_WORDS];   // row ci (candidate), word j / 32: collide(n_gt + ci, j)
    const int n = p.n_gt + p.n_s;
    const int nw = (n + 31) >> 5;
    for (int i = (int)threadIdx.x; i < n; i += AUG_THREADS) {
#pragma clang fp contract(off)
        const float* b = p.boxes + (int64_t)i * p.D;
        const float hx = b[3] * 0.5f, hy = b[4] * 0.5f;
        const float c = cosf(b[6]), s = sinf(b[6]);
        float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float lx = (k < 2) ? -hx : hx;
            const float ly = (k == 0 || k == 3) ? -hy : hy;
            const float xc = lx * c, ys = ly * s, xs = lx * s, yc = ly * c;
            const float X = (xc - ys) + b[0];
            const float Y = (xs + yc) + b[1];
            cor[i][2 * k] = X, cor[i][2 * k + 1] = Y;
            x0 = k ? fminf(x0, X) : X, x1 = k ? fmaxf(x1, X) : X;
            y0 = k ? fminf(y0, Y) : Y, y1 = k ? fmaxf(y1, Y) : Y;
        }
        su[i][0] = x0, su[i][1] = y0, su[i][2] = x1, su[i][3] = y1;
    }
    __syncthreads();
    for (int wd = (int)threadIdx.x; wd < p.n_s * nw; wd += AUG_THREADS) {
        const int ci = wd / nw, jw = wd - ci * nw;
        const int i = p.n_gt + ci;
        unsigned bits = 0;
        for (int t = 0; t < 32; ++t) {
            const int j = jw * 32 + t;
            if (j < n && j != i && gtc_collide(cor[i], cor[j], su[i], su[j])) bits |= 1u << t;
        }
        mat[ci * GT_WORDS + jw] = bits;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    // the greedy loop: lane l holds word l of the live set
    const int lane = (int)threadIdx.x;
    unsigned live = lane < GT_WORDS ? gtc_range_bits(0, p.n_gt, lane) : 0u;
    int kept = 0;
    for (int ci = 0; ci < p.n_s; ++ci) {
        if (ci == 0 || ((p.first[ci >> 5] >> (ci & 31)) & 1u)) {   // a new group: its candidates become live
            int end = ci + 1;
            while (end < p.n_s && !((p.first[end >> 5] >> (end & 31)) & 1u)) ++end;
            if (lane < GT_WORDS) live |= gtc_range_bits(p.n_gt + ci, p.n_gt + end, lane);
        }
        const unsigned hit = lane < nw ? (mat[ci * GT_WORDS + lane] & live) : 0u;
        const bool rejected = __ballot(hit != 0u) != 0ull;
        const int i = p.n_gt + ci;
        if (rejected) {
            if (lane == (i >> 5)) live &= ~(1u << (i & 31));
        } else {
            ++kept;
        }
        if (lane == 0) p.keep[ci] = rejected ? 0 : 1;
    }
    if (lane == 0) *p.count = kept;
}

// ---- host ---------------------------------------------------------------------------------------------------
extern "C" int64_t cmt_gtdb_extract_args_size(void) { return (int64_t)sizeof(cmt_gtdb_extract_args); }
extern "C" int64_t cmt_gtdb_gather_args_size(void) { return (int64_t)sizeof(cmt_gtdb_gather_args); }
extern "C" int64_t cmt_gtdb_collide_args_size(void) { return (int64_t)sizeof(cmt_gtdb_collide_args); }

extern "C" int64_t cmt_gtdb_extract_workspace_bytes(int64_t N, int M) {
    if (N <= 0 || M <= 0) return 0;
    return 2 * cdiv64(N, AUG_T) * (int64_t)M * (int64_t)sizeof(int);
}

extern "C" int cmt_gtdb_extract(const cmt_gtdb_extract_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_gtdb_extract: null argument struct");
    CMT_REQUIRE(a->N >= 0 && a->N < ((int64_t)1 << 31), "cmt_gtdb_extract: N must be in [0, 2^31)");
    CMT_REQUIRE(a->M >= 0 && a->M <= CMT_GTDB_MAX_BOXES, "cmt_gtdb_extract: M must be 0..1024");
    CMT_REQUIRE(a->N * (int64_t)a->M < ((int64_t)1 << 31), "cmt_gtdb_extract: N * M must be below 2^31");
    CMT_REQUIRE(a->F >= 3 && a->F <= 8, "cmt_gtdb_extract: F must be 3..8");
    CMT_REQUIRE(a->D == 7 || a->D == 9, "cmt_gtdb_extract: D must be 7 or 9");
    CMT_REQUIRE(a->cap >= 0 && a->cap < ((int64_t)1 << 31), "cmt_gtdb_extract: cap must be in [0, 2^31)");
    const int64_t need = cmt_gtdb_extract_workspace_bytes(a->N, a->M);
    CMT_REQUIRE(a->workspace_bytes >= need, "cmt_gtdb_extract: workspace below cmt_gtdb_extract_workspace_bytes(N, M)");
    if (a->N > 0) CMT_REQUIRE(ptr_aligned(a->points, 4), "cmt_gtdb_extract: points must be non-null and 4-byte aligned");
    if (a->M > 0) CMT_REQUIRE(ptr_aligned(a->boxes, 4), "cmt_gtdb_extract: boxes must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned(a->offsets, 4), "cmt_gtdb_extract: offsets must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->count_in, 4) && ptr_aligned_or_null(a->rows, 4), "cmt_gtdb_extract: count_in and rows must be 4-byte aligned");
    if (a->cap > 0) CMT_REQUIRE(a->rows != nullptr, "cmt_gtdb_extract: rows must be non-null with cap > 0");
    if (need > 0) CMT_REQUIRE(ptr_aligned(a->workspace, 4), "cmt_gtdb_extract: workspace must be non-null and 4-byte aligned");
    gtx_p p;
    p.pts = (const float*)a->points;
    p.count_in = a->count_in;
    p.boxes = (const float*)a->boxes;
    p.rows = (float*)a->rows;
    p.offsets = a->offsets;
    p.N = (unsigned)a->N;
    p.M = a->M, p.F = a->F, p.D = a->D;
    p.tiles = a->M > 0 ? (int)cdiv64(a->N, AUG_T) : 0;
    p.cnt = (int*)a->workspace;
    p.base = p.cnt ? p.cnt + (int64_t)p.tiles * p.M : nullptr;
    p.cap = a->cap;
    const hipStream_t st = (hipStream_t)stream;
    if (p.tiles > 0) gtdb_count_kernel<<<dim3((unsigned)p.tiles), AUG_THREADS, 0, st>>>(p);
    gtdb_scan_kernel<<<dim3(1), AUG_THREADS, 0, st>>>(p);   // with no pair it still writes the zero offsets
    if (p.tiles > 0 && p.cap > 0) gtdb_scatter_kernel<<<dim3((unsigned)p.tiles), AUG_THREADS, 0, st>>>(p);
    return cmt_check_launch("cmt_gtdb_extract");
}

extern "C" int cmt_gtdb_gather(const cmt_gtdb_gather_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_gtdb_gather: null argument struct");
    CMT_REQUIRE(a->K >= 0 && a->K <= CMT_AUG_MAX_BOXES, "cmt_gtdb_gather: K must be 0..128");
    CMT_REQUIRE(a->F >= 3 && a->F <= 8, "cmt_gtdb_gather: F must be 3..8");
    CMT_REQUIRE(a->n_rows >= 0 && a->n_rows < ((int64_t)1 << 31) && a->n_dst >= 0 && a->n_dst < ((int64_t)1 << 31),
                "cmt_gtdb_gather: n_rows and n_dst must be in [0, 2^31)");
    CMT_REQUIRE(ptr_aligned_or_null(a->rows, 4) && ptr_aligned_or_null(a->dst, 4) && ptr_aligned_or_null(a->seg_offset, 4) && ptr_aligned_or_null(a->seg_len, 4) &&
                    ptr_aligned_or_null(a->dst_offset, 4) && ptr_aligned_or_null(a->centre, 4),
                "cmt_gtdb_gather: every buffer must be 4-byte aligned");
    if (a->K == 0) return 0;
    CMT_REQUIRE(a->seg_offset && a->seg_len && a->dst_offset && a->centre,
                "cmt_gtdb_gather: seg_offset, seg_len, dst_offset and centre must be non-null with K > 0");
    if (a->n_rows == 0 || a->n_dst == 0) return 0;
    CMT_REQUIRE(a->rows && a->dst, "cmt_gtdb_gather: rows and dst must be non-null with rows to move");
    gtg_p p;
    p.rows = (const float*)a->rows;
    p.seg_offset = a->seg_offset, p.seg_len = a->seg_len, p.dst_offset = a->dst_offset;
    p.centre = (const float*)a->centre;
    p.dst = (float*)a->dst;
    p.n_rows = a->n_rows, p.n_dst = a->n_dst;
    p.F = a->F;
    int64_t gx = cdiv64(a->n_dst, AUG_THREADS);
    gx = gx < 1 ? 1 : (gx > 16 ? 16 : gx);
    gtdb_gather_kernel<<<dim3((unsigned)gx, (unsigned)a->K), AUG_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_gtdb_gather");
}

extern "C" int cmt_gtdb_collide(const cmt_gtdb_collide_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_gtdb_collide: null argument struct");
    CMT_REQUIRE(a->n_gt >= 0 && a->n_s >= 0 && (int64_t)a->n_gt + a->n_s <= CMT_GTDB_MAX_COLLIDE,
                "cmt_gtdb_collide: n_gt and n_s must not be negative and n_gt + n_s at most 512");
    CMT_REQUIRE(a->D == 7 || a->D == 9, "cmt_gtdb_collide: D must be 7 or 9");
    gtc_p p;
    for (int k = 0; k < GT_WORDS; ++k) p.first[k] = 0u;
    if (a->n_s > 0) {
        CMT_REQUIRE(a->group != nullptr, "cmt_gtdb_collide: group must be non-null with n_s > 0");
        for (int i = 0; i < a->n_s; ++i) {
            if (i > 0) CMT_REQUIRE(a->group[i] >= a->group[i - 1], "cmt_gtdb_collide: group must not decrease");
            if (i == 0 || a->group[i] != a->group[i - 1]) p.first[i >> 5] |= 1u << (i & 31);
        }
    }
    CMT_REQUIRE(ptr_aligned(a->count, 4), "cmt_gtdb_collide: count must be non-null and 4-byte aligned");
    if (a->n_gt + a->n_s > 0) CMT_REQUIRE(ptr_aligned(a->boxes, 4), "cmt_gtdb_collide: boxes must be non-null and 4-byte aligned");
    if (a->n_s > 0) CMT_REQUIRE(ptr_aligned(a->keep, 4), "cmt_gtdb_collide: keep must be non-null and 4-byte aligned");
    p.boxes = (const float*)a->boxes;
    p.keep = a->keep;
    p.count = a->count;
    p.n_gt = a->n_gt, p.n_s = a->n_s, p.D = a->D;
    gtdb_collide_kernel<<<dim3(1), AUG_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_gtdb_collide");
}
