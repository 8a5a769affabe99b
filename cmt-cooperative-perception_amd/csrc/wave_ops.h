// The wave and workgroup primitives of the data-path kernels (ptsprep, ptsaug, gtdb, track, boxiou, deteval), one
// copy each.  decode.hip, voxelize.hip and sparse.hip keep their own scans: they are on the frame's hot path.
#pragma once
#include "cmt_common.h"

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// lanes below this one whose bit is set in a ballot
__device__ __forceinline__ int wave_rank(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ int wave_shfl_up(int v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ double wave_shfl_up(double v, int d) {
    const long long bits = __double_as_longlong(v);
    const int hi = __shfl_up((int)(bits >> 32), d, 64), lo = __shfl_up((int)(uint32_t)bits, d, 64);
    return __longlong_as_double(((long long)hi << 32) | (long long)(uint32_t)lo);
}

// inclusive scan over the wave's lanes; every step adds as (lanes before) + (this lane's run): deteval's float64
// curves depend on that association
template <typename V>
__device__ __forceinline__ V wave_scan_incl(V run) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V o = wave_shfl_up(run, d);
        if (lane >= d) run = o + run;
    }
    return run;
}

constexpr unsigned QNAN32 = 0x7fc00000u;   // the quiet NaN of every padded tail

__device__ __forceinline__ bool finite32(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

// v into [0, hi]
template <typename I>
__device__ __forceinline__ int clamp_index(I v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// an optional device count word: null gives cap, negative 0, above cap gives cap.  cap must be below 2^31 (every
// caller's host checks see to it): it is narrowed to int before the clamp.
__device__ __forceinline__ int clamp_count(const int* word, int64_t cap) {
    return word == nullptr ? (int)cap : clamp_index(*word, (int)cap);
}

// ~ord(score): ascending in this value is descending in the score; -0 counts as +0.  Not for a NaN.
__device__ __forceinline__ uint32_t score_desc_key(float s) {
    uint32_t u = __float_as_uint(s + 0.f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

// Ordered compaction by one workgroup of 256 threads: flag[it] belongs to entry it * 256 + tid, so the 64 lanes of a
// wave hold 64 consecutive entries.  rank[it] becomes the number of flagged entries before it, the return value
// their total.  tab: ITERS * 4 LDS words.  Every thread calls it.  The two phases are for a caller that has a
// barrier of its own to share: post, ONE barrier, finish.
template <int ITERS>
__device__ __forceinline__ void tile_rank_post(const bool (&flag)[ITERS], int (&rank)[ITERS], int* tab) {
    const int lane = (int)threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const unsigned long long m = __ballot(flag[it]);
        rank[it] = wave_rank(m);
        if (lane == 0) tab[it * 4 + w] = __popcll(m);
    }
}

template <int ITERS>
__device__ __forceinline__ int tile_rank_finish(int (&rank)[ITERS], const int* tab) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int total = 0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int c = tab[it * 4 + v];
            if (v == w) rank[it] += total;
            total += c;
        }
    }
    return total;
}

template <int ITERS>
__device__ __forceinline__ int tile_rank(const bool (&flag)[ITERS], int (&rank)[ITERS], int* tab) {
    __syncthreads();   // the table's previous use has been read
    tile_rank_post<ITERS>(flag, rank, tab);
    __syncthreads();
    return tile_rank_finish<ITERS>(rank, tab);
}

// The two launches of an order-preserving stream compaction over tiles of TILE_T consecutive slots (cmt_pts_prepare,
// cmt_pts_augment).  row(slot, o): the keep predicate of a slot and, in o[0 .. F), its output row; both launches
// evaluate the same function, so the counts of the first are the ranks of the second.  No workgroup waits for
// another.
constexpr int TILE_T = 1024;
constexpr int TILE_THREADS = 256;
constexpr int TILE_R = TILE_T / TILE_THREADS;

// the count launch: the tile's kept rows -> tile_cnt[tile]
template <typename Row>
__device__ __forceinline__ void compact_count(int* tile_cnt, Row row) {
    __shared__ int part[TILE_THREADS / 64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned s0 = blockIdx.x * (unsigned)TILE_T + threadIdx.x;
    int kept = 0;
#pragma unroll
    for (int r = 0; r < TILE_R; ++r) {
        float o[8];
        kept += __popcll(__ballot(row(s0 + (unsigned)(r * TILE_THREADS), o)));
    }
    if (lane == 0) part[w] = kept;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// the scatter launch: kept rows to dst[rank][0 .. F) in slot order, quiet NaN in the rows of the tile's own index
// range at or beyond the total (scatter targets lie below the total, fill targets at or beyond it: no element has
// two writers), the total to *count.  The tile_cnt reduction and the rank table share one barrier.
template <typename Row>
__device__ __forceinline__ void compact_scatter(const int* tile_cnt, int tiles, float* dst, int* count, unsigned n_out, int F,
                                                Row row) {
    __shared__ int part[2][TILE_THREADS / 64];
    __shared__ int tab[TILE_R * 4];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = (int)blockIdx.x;
    int before = 0, total = 0;
    for (int t = (int)threadIdx.x; t < tiles; t += TILE_THREADS) {
        const int c = tile_cnt[t];
        total += c;
        before += t < b ? c : 0;
    }
    before = wave_sum(before);
    total = wave_sum(total);
    if (lane == 0) part[0][w] = before, part[1][w] = total;

    const unsigned s0 = (unsigned)b * (unsigned)TILE_T + threadIdx.x;
    float o[TILE_R][8];
    bool keep[TILE_R];
    int rank[TILE_R];
#pragma unroll
    for (int r = 0; r < TILE_R; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[r][j] = 0.f;
        keep[r] = row(s0 + (unsigned)(r * TILE_THREADS), o[r]);
    }
    tile_rank_post<TILE_R>(keep, rank, tab);
    __syncthreads();
    before = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    total = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (b == 0 && threadIdx.x == 0) *count = total;
    tile_rank_finish<TILE_R>(rank, tab);
#pragma unroll
    for (int r = 0; r < TILE_R; ++r) {
        const unsigned i = s0 + (unsigned)(r * TILE_THREADS);
        const unsigned g = (unsigned)(before + rank[r]);   // below total <= n_out: both launches evaluate the same function
        if (keep[r] && g < n_out) {
            float* q = dst + (int64_t)g * F;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < F) q[j] = o[r][j];
        }
        if (i < n_out && i >= (unsigned)total) {
            unsigned* q = (unsigned*)dst + (int64_t)i * F;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < F) q[j] = QNAN32;
        }
    }
}
