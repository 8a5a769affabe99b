// cmt_pts_prepare: one cloud's raw sweep rows (fp32 [n][load_dim], S segments) -> the detector's points
// (fp32 [n][F_out], kept rows first in input order, the rest quiet NaN) and the kept count, on the device:
// remove_close, the float64 sweep transform, the time column, the column selection, the float32 agent
// transform and the strict range filter of include/cmt_hip.h, as an order-preserving stream compaction.
//
// Two launches, no workgroup waits for another, over tiles of PTS_T consecutive rows, a wave's 64 lanes on 64
// consecutive rows (a chunk), with pts_row as the row function of both: the count launch is wave_ops.h's
// compact_count, the scatter launch keeps its own copy of compact_scatter's body (see pts_scatter_kernel).
// The segment's parameters stay scalar: a chunk loops over the segments that overlap its 64 rows (one, at
// a segment boundary two or more) and the rows of that segment are evaluated under the loop.  Rows are read
// with dword loads (a load_dim = 5 row is 20 bytes).  Contraction is off for the row function (and for the
// file, see the Makefile): the contract's products and sums are separate roundings.
#include "wave_ops.h"

#include <cmath>

constexpr int PTS_T = TILE_T;         // rows per tile
constexpr int PTS_THREADS = TILE_THREADS;
constexpr int PTS_R = TILE_R;
constexpr int PTS_CHUNKS = PTS_T / 64;

struct pts_p {
    const float* src;
    float* dst;
    int* count;
    int* tile_cnt;       // the workspace: kept rows of each tile
    unsigned n;
    int tiles, S, load_dim, F;
    int use_dim[8];
    int has_agent, has_range;
    float rot32[9], trans32[3], range[6];
    unsigned seg_start[CMT_PTS_MAX_SEG + 1];
    cmt_pts_segment seg[CMT_PTS_MAX_SEG];
};

// One row of segment sg: the keep predicate and, in o[0 .. F), the output row.  Both kernels call this.
__device__ __forceinline__ bool pts_eval(const pts_p& p, const cmt_pts_segment& sg, const float* r, float (&o)[8]) {
#pragma clang fp contract(off)
    const float x = r[0], y = r[1], z = r[2];
    const float cr = sg.close_radius;
    bool keep = !(__builtin_fabsf(x) < cr && __builtin_fabsf(y) < cr);   // cr == 0: nothing is below it
    float c[3] = {x, y, z};
    if (sg.has_sweep_xform) {
        const double dx = (double)x, dy = (double)y, dz = (double)z;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double m0 = dx * sg.rot[3 * k], m1 = dy * sg.rot[3 * k + 1], m2 = dz * sg.rot[3 * k + 2];
            const float q = (float)((m0 + m1) + m2);
            c[k] = (float)((double)q + sg.trans[k]);
        }
    }
    const int tc = sg.time_col;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (tc == k) c[k] = sg.time_val;
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = c[j];
#pragma unroll
    for (int j = 3; j < 8; ++j) {
        if (j < p.F) {
            const int u = p.use_dim[j];   // scalar
            float v;
            if (u == tc)
                v = sg.time_val;
            else if (u < 3)
                v = u == 0 ? c[0] : (u == 1 ? c[1] : c[2]);
            else
                v = r[u];
            o[j] = v;
        }
    }
    if (p.has_agent) {
        const float a = o[0], b = o[1], d = o[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float m0 = a * p.rot32[3 * k], m1 = b * p.rot32[3 * k + 1], m2 = d * p.rot32[3 * k + 2];
            o[k] = ((m0 + m1) + m2) + p.trans32[k];
        }
    }
    if (p.has_range) {
#pragma unroll
        for (int k = 0; k < 3; ++k) keep = keep && o[k] > p.range[k] && o[k] < p.range[3 + k];
    }
    return keep;
}

// the first row of row i's chunk, as a scalar: the 64 lanes of a wave hold one chunk
__device__ __forceinline__ unsigned pts_chunk(unsigned i) { return (unsigned)__builtin_amdgcn_readfirstlane((int)(i & ~63u)); }

// row i of the chunk that starts at row c0 (wave-uniform): false for a row at or beyond n
__device__ __forceinline__ bool pts_row(const pts_p& p, unsigned c0, unsigned i, float (&o)[8]) {
    bool keep = false;
    const unsigned c1 = c0 + 64u;
    for (int s = 0; s < p.S; ++s) {
        const unsigned lo = p.seg_start[s], hi = p.seg_start[s + 1];
        if (hi <= c0 || lo >= c1) continue;   // no row of this chunk
        if (i >= lo && i < hi) keep = pts_eval(p, p.seg[s], p.src + (int64_t)i * p.load_dim, o);
    }
    return keep;
}

__global__ __launch_bounds__(PTS_THREADS) void pts_count_kernel(pts_p p) {
    compact_count(p.tile_cnt, [&](unsigned i, float (&o)[8]) { return pts_row(p, pts_chunk(i), i, o); });
}

// Its own copy of compact_scatter's body (wave_ops.h), kept on purpose: on the shared body pts_row's per-chunk scalar
// state (the segment loop of four chunks) stays live across the barrier and the kernel's SGPR spills go from 38 to 108,
// which costs the two launches about a microsecond.  Here the chunk table is walked in chunk order and a chunk is
// stored as the walk reaches it.  Same contract: rank, bounded store g < n, NaN tail, one writer of *count.
__global__ __launch_bounds__(PTS_THREADS) void pts_scatter_kernel(pts_p p) {
    __shared__ int part[2][PTS_THREADS / 64];
    __shared__ int chunk[PTS_CHUNKS];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = (int)blockIdx.x;
    int before = 0, total = 0;
    for (int t = (int)threadIdx.x; t < p.tiles; t += PTS_THREADS) {
        const int c = p.tile_cnt[t];
        total += c;
        before += t < b ? c : 0;
    }
    before = wave_sum(before);
    total = wave_sum(total);
    if (lane == 0) part[0][w] = before, part[1][w] = total;

    const unsigned t0 = (unsigned)b * (unsigned)PTS_T;
    float o[PTS_R][8];
    bool keep[PTS_R];
    int rank[PTS_R];
#pragma unroll
    for (int r = 0; r < PTS_R; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[r][j] = 0.f;
        const unsigned c0 = t0 + (unsigned)((r * 4 + w) * 64);
        keep[r] = pts_row(p, c0, c0 + (unsigned)lane, o[r]);
        const unsigned long long m = __ballot(keep[r]);
        rank[r] = wave_rank(m);
        if (lane == 0) chunk[r * 4 + w] = __popcll(m);
    }
    __syncthreads();
    before = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    total = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (b == 0 && threadIdx.x == 0) *p.count = total;

    int run = before;   // kept rows in front of chunk c
#pragma unroll
    for (int c = 0; c < PTS_CHUNKS; ++c) {
        if ((c & 3) == w) {
            const int r = c >> 2;
            const unsigned i = t0 + (unsigned)(c * 64 + lane);
            const unsigned g = (unsigned)(run + rank[r]);   // below total <= n: both launches evaluate the same function
            if (keep[r] && g < p.n) {
                float* q = p.dst + (int64_t)g * p.F;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < p.F) q[j] = o[r][j];
            }
            if (i < p.n && i >= (unsigned)total) {
                unsigned* q = (unsigned*)p.dst + (int64_t)i * p.F;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < p.F) q[j] = QNAN32;
            }
        }
        run += chunk[c];
    }
}

extern "C" int64_t cmt_pts_prepare_args_size(void) { return (int64_t)sizeof(cmt_pts_prepare_args); }

extern "C" int cmt_pts_prepare_tile_rows(void) { return PTS_T; }

extern "C" int64_t cmt_pts_prepare_workspace_bytes(int64_t n_total) {
    if (n_total <= 0) return 0;
    return cdiv64(n_total, PTS_T) * (int64_t)sizeof(int);
}

extern "C" int cmt_pts_prepare(const cmt_pts_prepare_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_pts_prepare: null argument struct");
    CMT_REQUIRE(a->S >= 1 && a->S <= CMT_PTS_MAX_SEG, "cmt_pts_prepare: S must be 1..16");
    CMT_REQUIRE(a->load_dim >= 3 && a->load_dim <= 8, "cmt_pts_prepare: load_dim must be 3..8");
    CMT_REQUIRE(a->F_out >= 3 && a->F_out <= 8, "cmt_pts_prepare: F_out must be 3..8");
    CMT_REQUIRE(a->n_total >= 0 && a->n_total < ((int64_t)1 << 31), "cmt_pts_prepare: n_total must be in [0, 2^31)");
    for (int j = 0; j < a->F_out; ++j)
        CMT_REQUIRE(a->use_dim[j] >= 0 && a->use_dim[j] < a->load_dim, "cmt_pts_prepare: use_dim entry outside [0, load_dim)");
    CMT_REQUIRE(a->use_dim[0] == 0 && a->use_dim[1] == 1 && a->use_dim[2] == 2, "cmt_pts_prepare: use_dim must start with 0, 1, 2");
    CMT_REQUIRE(a->seg_start[0] == 0, "cmt_pts_prepare: seg_start[0] must be 0");
    for (int s = 0; s < a->S; ++s)
        CMT_REQUIRE(a->seg_start[s + 1] >= a->seg_start[s], "cmt_pts_prepare: seg_start must not decrease");
    CMT_REQUIRE(a->seg_start[a->S] == a->n_total, "cmt_pts_prepare: seg_start[S] must equal n_total");
    for (int s = 0; s < a->S; ++s) {
        const cmt_pts_segment& g = a->seg[s];
        CMT_REQUIRE(g.time_col >= -1 && g.time_col < a->load_dim, "cmt_pts_prepare: time_col must be -1 or below load_dim");
        CMT_REQUIRE(std::isfinite(g.close_radius) && g.close_radius >= 0.f, "cmt_pts_prepare: close_radius must be finite and >= 0");
        if (g.has_sweep_xform) {
            for (int k = 0; k < 9; ++k) CMT_REQUIRE(std::isfinite(g.rot[k]), "cmt_pts_prepare: non-finite sweep rotation");
            for (int k = 0; k < 3; ++k) CMT_REQUIRE(std::isfinite(g.trans[k]), "cmt_pts_prepare: non-finite sweep translation");
        }
    }
    if (a->has_agent_xform) {
        for (int k = 0; k < 9; ++k) CMT_REQUIRE(std::isfinite(a->rot32[k]), "cmt_pts_prepare: non-finite agent rotation");
        for (int k = 0; k < 3; ++k) CMT_REQUIRE(std::isfinite(a->trans32[k]), "cmt_pts_prepare: non-finite agent translation");
    }
    if (a->has_range) {
        for (int k = 0; k < 6; ++k) CMT_REQUIRE(std::isfinite(a->range[k]), "cmt_pts_prepare: non-finite range");
        for (int k = 0; k < 3; ++k) CMT_REQUIRE(a->range[k] < a->range[3 + k], "cmt_pts_prepare: range min must be below max");
    }
    CMT_REQUIRE(a->count != nullptr, "cmt_pts_prepare: count must be non-null");
    CMT_REQUIRE(ptr_aligned_or_null(a->count, 4), "cmt_pts_prepare: count must be 4-byte aligned");
    const int64_t need = cmt_pts_prepare_workspace_bytes(a->n_total);
    if (a->n_total > 0) {
        CMT_REQUIRE(a->src && a->dst && a->workspace, "cmt_pts_prepare: src, dst and workspace must be non-null");
        CMT_REQUIRE(ptr_aligned_or_null(a->src, 4) && ptr_aligned_or_null(a->dst, 4) && ptr_aligned_or_null(a->workspace, 4),
                    "cmt_pts_prepare: src, dst and workspace must be 4-byte aligned");
        CMT_REQUIRE(a->workspace_bytes >= need, "cmt_pts_prepare: workspace below cmt_pts_prepare_workspace_bytes(n_total)");
    }
    pts_p p;
    p.src = (const float*)a->src;
    p.dst = (float*)a->dst;
    p.count = a->count;
    p.tile_cnt = (int*)a->workspace;
    p.n = (unsigned)a->n_total;
    p.tiles = (int)cdiv64(a->n_total, PTS_T);
    p.S = a->S, p.load_dim = a->load_dim, p.F = a->F_out;
    for (int j = 0; j < 8; ++j) p.use_dim[j] = j < a->F_out ? a->use_dim[j] : 0;
    p.has_agent = a->has_agent_xform ? 1 : 0;
    p.has_range = a->has_range ? 1 : 0;
    for (int k = 0; k < 9; ++k) p.rot32[k] = a->rot32[k];
    for (int k = 0; k < 3; ++k) p.trans32[k] = a->trans32[k];
    for (int k = 0; k < 6; ++k) p.range[k] = a->range[k];
    for (int s = 0; s <= CMT_PTS_MAX_SEG; ++s) p.seg_start[s] = (unsigned)a->seg_start[s <= a->S ? s : a->S];
    for (int s = 0; s < CMT_PTS_MAX_SEG; ++s) p.seg[s] = a->seg[s < a->S ? s : 0];
    const hipStream_t st = (hipStream_t)stream;
    if (p.tiles > 0) pts_count_kernel<<<dim3((unsigned)p.tiles), PTS_THREADS, 0, st>>>(p);
    // with no rows one workgroup still writes count = 0
    pts_scatter_kernel<<<dim3((unsigned)(p.tiles > 0 ? p.tiles : 1)), PTS_THREADS, 0, st>>>(p);
    return cmt_check_launch("cmt_pts_prepare");
}
