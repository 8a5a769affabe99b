// Detection evaluation on the device: the nuScenes-style matching, curves, AP and TP errors of
// include/cmt_hip.h (cmt_det_eval_*).  Float64 on float32 inputs, no contraction anywhere in this file (see
// the Makefile): every comparison of the contract sees separately rounded products and sums.
//
//   det_keys_kernel   one thread per row: the filters and the three int64 sort keys.  The caller sorts them
//                     (stable, ascending) between this launch and the next.
//   det_match_kernel  one wave per (sample, class).  The sample-major sort makes the pair's predictions one
//                     contiguous run in visiting order and its ground truth one contiguous run in annotation
//                     order; both runs are found by binary search.  Lane g owns ground truth g, g + 64, ...:
//                     the first 64 live in registers with their taken bits (one per threshold), further
//                     chunks keep their bits in the workspace, each byte read and written by its own lane only.
//                     Per prediction the distances are computed once, the per-threshold minima differ only in
//                     the taken mask: one lexicographic (distance bits, annotation index) wave minimum by
//                     xor-shuffles per threshold, then the winner lane sets its bit and writes the row.
//                     The same launch has C workgroups that count npos and a few that fill the rows of
//                     predictions that do not exist or were filtered: every output element has one writer.
//   det_curve_kernel  one workgroup per (class, threshold) over the class's run of the class-major order:
//                     integer block scan of tp (exact) with the order-preserving compaction of the matches,
//                     the two 101-point resamplings by binary search, per error the NaN-aware cumulative mean
//                     as a fixed-tree float64 scan and the reversed resampling, then calc_ap / calc_tp.
//   det_match_iou_kernel  the same wave per (sample, class) with the rotated-box IoU of box_overlap.h (float32, the
//                     ground truth as the first box) in place of the centre distance and the largest value in place
//                     of the smallest.  The derived box of the lane's first ground truth stays in registers, the
//                     prediction's is derived once per prediction, the clip runs once per (prediction, lane) in the
//                     lane's LDS slot; the thresholds differ only in the taken mask.
//   det_ap_interp_kernel  one workgroup per (class, threshold): the precision envelope at the matches as a reverse
//                     running maximum, then the all-point AP and the 40-point AP as serial sums.
#include "box_overlap.h"
#include "wave_ops.h"

#include <cmath>
#include <cstdint>

constexpr int DET_THREADS = 256;
constexpr int DET_WAVES = DET_THREADS / 64;
constexpr int DET_PER = 8;                          // consecutive scan terms per thread
constexpr int DET_CHUNK = DET_THREADS * DET_PER;    // scan terms per workgroup step
constexpr int DET_NE = CMT_DET_NELEM;
constexpr int DET_FILL_BLOCKS = 64;
constexpr int64_t DET_NONE = INT64_MAX;

struct det_p {
    int64_t N, G;
    int S, C, T, tp_index, first_ind;
    int64_t match_blocks;
    double range[CMT_DET_MAX_CLASSES], period[CMT_DET_MAX_CLASSES], th[CMT_DET_MAX_THRESHOLDS];
    double min_precision;
    const float *pbox, *pscore, *gbox;
    const int *plabel, *psample, *glabel, *gsample, *gnum, *n_pred, *n_gt;
    int64_t *key_class, *key_sample, *key_gt;
    const int64_t *sk_class, *si_class, *sk_sample, *si_sample, *sk_gt, *si_gt;
    unsigned char* tp;
    int* match_gt;
    double* err;
    int* npos;
    double *md, *ap, *tp_err;
    double* ws_cm;           // [T][N] cumulative mean of one error, reused by the four
    int* ws_ctp;             // [T][N] running tp count
    int* ws_mpos;            // [T][N] class-run position of the m-th match
    unsigned char* ws_taken; // [G] taken bits of ground truth beyond the first 64 of a (sample, class)
    float* match_iou;        // [T][N], the IoU match only (else null)
};

struct det_iou_p {
    float th[CMT_DET_MAX_THRESHOLDS];
    float z_origin;
    int use_3d;
    double* ap_interp;
};
static_assert(DET_THREADS == BI_THREADS, "a lane of the match workgroup owns one clip slot");

__device__ __forceinline__ double det_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ int64_t det_lower_bound(const int64_t* k, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (k[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(DET_THREADS) void det_keys_kernel(det_p p) {
    const int64_t i = (int64_t)blockIdx.x * DET_THREADS + threadIdx.x;
    if (i < p.N) {
        int64_t kc = DET_NONE, ks = DET_NONE;
        if (i < clamp_count(p.n_pred, p.N)) {
            const int c = p.plabel[i], s = p.psample[i];
            if (c >= 0 && c < p.C && s >= 0 && s < p.S) {
                const double x = (double)p.pbox[i * 9], y = (double)p.pbox[i * 9 + 1];
                const double xx = x * x, yy = y * y;
                if (sqrt(xx + yy) < p.range[c]) {
                    const int64_t sk = (int64_t)score_desc_key(p.pscore[i]);
                    kc = ((int64_t)c << 32) | sk;
                    ks = ((((int64_t)s << 6) | (int64_t)c) << 32) | sk;
                }
            }
        }
        p.key_class[p.N - 1 - i] = kc;
        p.key_sample[p.N - 1 - i] = ks;
    }
    if (i < p.G) {
        int64_t kg = DET_NONE;
        if (i < clamp_count(p.n_gt, p.G)) {
            const int c = p.glabel[i], s = p.gsample[i];
            if (c >= 0 && c < p.C && s >= 0 && s < p.S && p.gnum[i] != 0) {
                const double x = (double)p.gbox[i * 9], y = (double)p.gbox[i * 9 + 1];
                const double xx = x * x, yy = y * y;
                if (sqrt(xx + yy) < p.range[c]) kg = ((int64_t)s << 6) | (int64_t)c;
            }
        }
        p.key_gt[i] = kg;
    }
}

__device__ __forceinline__ double det_min_nan(double a, double b) {   // numpy.minimum
    double m = a < b ? a : b;
    if (b != b) m = b;
    if (a != a) m = a;
    return m;
}

// the four errors of prediction row i matched to ground-truth row g at centre distance d
__device__ __forceinline__ void det_errors(const det_p& p, int64_t i, int64_t g, int c, double d, double (&e)[4]) {
    const float* pb = p.pbox + i * 9;
    const float* gb = p.gbox + g * 9;
    e[0] = d;
    const double dvx = (double)pb[7] - (double)gb[7], dvy = (double)pb[8] - (double)gb[8];
    const double vxx = dvx * dvx, vyy = dvy * dvy;
    e[1] = sqrt(vxx + vyy);
    const double wg = gb[3], lg = gb[4], hg = gb[5], wp = pb[3], lp = pb[4], hp = pb[5];
    const double vg = (wg * lg) * hg, vp = (wp * lp) * hp;
    const double in = (det_min_nan(wg, wp) * det_min_nan(lg, lp)) * det_min_nan(hg, hp);
    const double un = (vg + vp) - in;
    e[2] = 1.0 - in / un;
    const double P = p.period[c], half = P / 2;
    const double a = ((double)gb[6] - (double)pb[6]) + half;
    double r = fmod(a, P);
    if (r < 0) r = r + P;
    double diff = r - half;
    const double pi = 3.141592653589793;
    if (diff > pi) diff = diff - 2 * pi;
    e[3] = fabs(diff);
}

// tp = 0 rows of prediction i for threshold t
__device__ __forceinline__ void det_write_miss(const det_p& p, int t, int64_t i) {
    p.tp[(int64_t)t * p.N + i] = 0;
    p.match_gt[(int64_t)t * p.N + i] = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) p.err[((int64_t)t * 4 + e) * p.N + i] = det_nan();
    if (p.match_iou) p.match_iou[(int64_t)t * p.N + i] = __uint_as_float(QNAN32);
}

__device__ __forceinline__ int det_block_sum(int v, int* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < DET_WAVES; ++w) s += part[w];
    return s;
}

// the workgroups behind the matching ones, x = 0 ..: C that count npos, DET_FILL_BLOCKS that fill the rows of
// predictions that take no part
__device__ __forceinline__ void det_match_rest(const det_p& p, int64_t x, int* part) {
    if (x < p.C) {   // npos of class x: kept ground truth sorts in front of the rest
        int n = 0;
        for (int64_t j = threadIdx.x; j < p.G; j += DET_THREADS) {
            const int64_t k = p.sk_gt[j];
            n += (k != DET_NONE && (int)(k & 63) == (int)x) ? 1 : 0;
        }
        n = det_block_sum(n, part);
        if (threadIdx.x == 0) p.npos[x] = n;
    } else {         // rows of predictions that take no part: they sort behind every kept one
        const int64_t first = det_lower_bound(p.sk_sample, p.N, DET_NONE);
        for (int64_t q = first + (x - p.C) * DET_THREADS + threadIdx.x; q < p.N;
             q += (int64_t)DET_FILL_BLOCKS * DET_THREADS) {
            const int64_t i = p.N - 1 - p.si_sample[q];
            for (int t = 0; t < p.T; ++t) det_write_miss(p, t, i);
        }
    }
}

__global__ __launch_bounds__(DET_THREADS) void det_match_kernel(det_p p) {
    __shared__ int part[DET_WAVES];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t b = blockIdx.x;
    if (b >= p.match_blocks) {
        det_match_rest(p, b - p.match_blocks, part);
        return;
    }
    const int64_t pair = b * DET_WAVES + w;
    if (pair >= (int64_t)p.S * p.C) return;
    const int c = (int)(pair % p.C);
    const int64_t sc = ((pair / p.C) << 6) | (int64_t)c;
    const int64_t g0 = det_lower_bound(p.sk_gt, p.G, sc), g1 = det_lower_bound(p.sk_gt, p.G, sc + 1);
    const int64_t p0 = det_lower_bound(p.sk_sample, p.N, sc << 32), p1 = det_lower_bound(p.sk_sample, p.N, (sc + 1) << 32);
    const int ng = (int)(g1 - g0);
    const int chunks = (ng + 63) >> 6;

    const bool have0 = lane < ng;
    const int64_t row0 = have0 ? p.si_gt[g0 + lane] : 0;
    const double gx0 = have0 ? (double)p.gbox[row0 * 9] : 0.0, gy0 = have0 ? (double)p.gbox[row0 * 9 + 1] : 0.0;
    unsigned taken0 = 0;
    for (int k = 1; k < chunks; ++k)
        if (k * 64 + lane < ng) p.ws_taken[g0 + k * 64 + lane] = 0;

    for (int64_t q = p0; q < p1; ++q) {
        const int64_t i = p.N - 1 - p.si_sample[q];
        const double px = (double)p.pbox[i * 9], py = (double)p.pbox[i * 9 + 1];
        uint64_t bk[CMT_DET_MAX_THRESHOLDS];
        int bpos[CMT_DET_MAX_THRESHOLDS];
#pragma unroll
        for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t) bk[t] = ~0ull, bpos[t] = INT32_MAX;
        if (have0) {
            const double dx = px - gx0, dy = py - gy0;
            const double xx = dx * dx, yy = dy * dy;
            const uint64_t key = (uint64_t)__double_as_longlong(sqrt(xx + yy));   // d >= 0: its bits order like d
#pragma unroll
            for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t)
                if (t < p.T && !((taken0 >> t) & 1u)) bk[t] = key, bpos[t] = lane;
        }
        for (int k = 1; k < chunks; ++k) {
            const int pos = k * 64 + lane;
            if (pos < ng) {
                const int64_t row = p.si_gt[g0 + pos];
                const unsigned tk = p.ws_taken[g0 + pos];
                const double dx = px - (double)p.gbox[row * 9], dy = py - (double)p.gbox[row * 9 + 1];
                const double xx = dx * dx, yy = dy * dy;
                const uint64_t key = (uint64_t)__double_as_longlong(sqrt(xx + yy));
#pragma unroll
                for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t)
                    if (t < p.T && !((tk >> t) & 1u) && key < bk[t]) bk[t] = key, bpos[t] = pos;   // strict: lowest index stays
            }
        }
#pragma unroll
        for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t) {
            if (t < p.T) {
                uint64_t k = bk[t];
                int pos = bpos[t];
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const uint64_t ok = ((uint64_t)(uint32_t)__shfl_xor((int)(k >> 32), d, 64) << 32) |
                                        (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)k, d, 64);
                    const int op = __shfl_xor(pos, d, 64);
                    if (ok < k || (ok == k && op < pos)) k = ok, pos = op;
                }
                const double dm = __longlong_as_double((long long)k);
                const bool match = pos != INT32_MAX && dm < p.th[t];
                if (match) {
                    if ((pos & 63) == lane) {   // the owner of the winner
                        if (pos < 64)
                            taken0 |= 1u << t;
                        else
                            p.ws_taken[g0 + pos] = (unsigned char)(p.ws_taken[g0 + pos] | (1u << t));
                        const int64_t row = p.si_gt[g0 + pos];
                        double e[4];
                        det_errors(p, i, row, c, dm, e);
                        p.tp[(int64_t)t * p.N + i] = 1;
                        p.match_gt[(int64_t)t * p.N + i] = (int)row;
#pragma unroll
                        for (int j = 0; j < 4; ++j) p.err[((int64_t)t * 4 + j) * p.N + i] = e[j];
                    }
                } else if (lane == 0) {
                    det_write_miss(p, t, i);
                }
            }
        }
    }
}

// ---- the IoU match --------------------------------------------------------------------------------------

// ~bits(iou) of ground truth Gt (the first box: the pair is clipped in its frame) and prediction P: iou >= 0, so
// ascending in this key is descending in the value.  An invalid box on either side gives 0, and so does a NaN
// quotient (0 / 0 of extents whose products underflow).  px, py: the lane's clip slot.
__device__ __forceinline__ uint32_t det_iou_key(const bi_box& Gt, const bi_box& P, int use_3d, float* px, float* py) {
    float v = 0.f;
    if (Gt.ok && P.ok) {
        float area, h;
        bi_pair(Gt, P, px, py, area, h);
        v = use_3d ? bi_3d(Gt, P, area, h) : bi_bev(Gt, P, area);
        if (!(v == v)) v = 0.f;
    }
    return ~__float_as_uint(v);
}

__global__ __launch_bounds__(DET_THREADS) void det_match_iou_kernel(det_p p, det_iou_p q) {
    __shared__ float px[2 * BI_SLOT], py[2 * BI_SLOT];
    __shared__ int part[DET_WAVES];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    if (b >= p.match_blocks) {
        det_match_rest(p, b - p.match_blocks, part);
        return;
    }
    const int64_t pair = b * DET_WAVES + w;
    if (pair >= (int64_t)p.S * p.C) return;
    const int c = (int)(pair % p.C);
    const int64_t sc = ((pair / p.C) << 6) | (int64_t)c;
    const int64_t g0 = det_lower_bound(p.sk_gt, p.G, sc), g1 = det_lower_bound(p.sk_gt, p.G, sc + 1);
    const int64_t p0 = det_lower_bound(p.sk_sample, p.N, sc << 32), p1 = det_lower_bound(p.sk_sample, p.N, (sc + 1) << 32);
    const int ng = (int)(g1 - g0);
    const int chunks = (ng + 63) >> 6;
    float* sx = px + tid;
    float* sy = py + tid;

    const bool have0 = lane < ng;
    const bi_box G0 = have0 ? bi_derive(p.gbox + p.si_gt[g0 + lane] * 9, q.z_origin) : bi_none();
    unsigned taken0 = 0;
    for (int k = 1; k < chunks; ++k)
        if (k * 64 + lane < ng) p.ws_taken[g0 + k * 64 + lane] = 0;

    for (int64_t v = p0; v < p1; ++v) {
        const int64_t i = p.N - 1 - p.si_sample[v];
        const bi_box P = bi_derive(p.pbox + i * 9, q.z_origin);
        uint32_t bk[CMT_DET_MAX_THRESHOLDS];
        int bpos[CMT_DET_MAX_THRESHOLDS];
#pragma unroll
        for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t) bk[t] = ~0u, bpos[t] = INT32_MAX;
        if (have0) {
            const uint32_t key = det_iou_key(G0, P, q.use_3d, sx, sy);
#pragma unroll
            for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t)
                if (t < p.T && !((taken0 >> t) & 1u)) bk[t] = key, bpos[t] = lane;
        }
        for (int k = 1; k < chunks; ++k) {
            const int pos = k * 64 + lane;
            if (pos < ng) {
                const bi_box Gk = bi_derive(p.gbox + p.si_gt[g0 + pos] * 9, q.z_origin);
                const unsigned tk = p.ws_taken[g0 + pos];
                const uint32_t key = det_iou_key(Gk, P, q.use_3d, sx, sy);
#pragma unroll
                for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t)   // strict, or the first candidate: the lowest index stays
                    if (t < p.T && !((tk >> t) & 1u) && (key < bk[t] || bpos[t] == INT32_MAX)) bk[t] = key, bpos[t] = pos;
            }
        }
#pragma unroll
        for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t) {
            if (t < p.T) {
                uint32_t k = bk[t];
                int pos = bpos[t];
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const uint32_t ok = (uint32_t)__shfl_xor((int)k, d, 64);
                    const int op = __shfl_xor(pos, d, 64);
                    if (ok < k || (ok == k && op < pos)) k = ok, pos = op;
                }
                const float iou = __uint_as_float(~k);
                const bool match = pos != INT32_MAX && iou > q.th[t];
                if (match) {
                    if ((pos & 63) == lane) {   // the owner of the winner
                        if (pos < 64)
                            taken0 |= 1u << t;
                        else
                            p.ws_taken[g0 + pos] = (unsigned char)(p.ws_taken[g0 + pos] | (1u << t));
                        const int64_t row = p.si_gt[g0 + pos];
                        const double dx = (double)p.pbox[i * 9] - (double)p.gbox[row * 9];
                        const double dy = (double)p.pbox[i * 9 + 1] - (double)p.gbox[row * 9 + 1];
                        const double xx = dx * dx, yy = dy * dy;
                        double e[4];
                        det_errors(p, i, row, c, sqrt(xx + yy), e);
                        p.tp[(int64_t)t * p.N + i] = 1;
                        p.match_gt[(int64_t)t * p.N + i] = (int)row;
#pragma unroll
                        for (int j = 0; j < 4; ++j) p.err[((int64_t)t * 4 + j) * p.N + i] = e[j];
                        if (p.match_iou) p.match_iou[(int64_t)t * p.N + i] = iou;
                    }
                } else if (lane == 0) {
                    det_write_miss(p, t, i);
                }
            }
        }
    }
}

// ---- curves -------------------------------------------------------------------------------------------

// inclusive scan over the workgroup's DET_CHUNK terms, thread-major: v[] in, inclusive prefix out; returns the
// chunk total.  Tree: the thread's 8 terms in order, shuffle-up scan of the 64 thread totals, the 4 wave totals
// in order.  part: DET_WAVES entries, free again after the call.
template <typename V>
__device__ __forceinline__ V det_block_scan(V (&v)[DET_PER], V* part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 1; j < DET_PER; ++j) v[j] = v[j - 1] + v[j];
    const V run = wave_scan_incl(v[DET_PER - 1]);   // the inclusive sum over the wave's threads up to this one, as o + run
    __syncthreads();   // part may still be read from the call before
    if (lane == 63) part[w] = run;
    __syncthreads();
    V before = (V)0, total = (V)0;
#pragma unroll
    for (int k = 0; k < DET_WAVES; ++k) {
        if (k == w) before = total;
        total = total + part[k];
    }
    V tb = wave_shfl_up(run, 1);   // the threads before in the wave
    if (lane == 0) tb = (V)0;
    const V base = before + tb;
#pragma unroll
    for (int j = 0; j < DET_PER; ++j) v[j] = base + v[j];
    return total;
}

// The running tp count ctp[0 .. n) and the positions mpos[0 .. M) of the matches of one (class, threshold), in
// visiting order (si: the class's run of the class-major order); returns M.  Integer block scans: exact.  Ends with
// a barrier, so every thread may read both arrays.
__device__ __forceinline__ int det_scan_tp(const det_p& p, const unsigned char* tp, const int64_t* si, int64_t n, int* ctp,
                                           int* mpos, int* ipart) {
    int M = 0;
    for (int64_t base = 0; base < n; base += DET_CHUNK) {
        int v[DET_PER];
        unsigned hit = 0;
        const int64_t j0 = base + (int64_t)threadIdx.x * DET_PER;
#pragma unroll
        for (int j = 0; j < DET_PER; ++j) {
            v[j] = j0 + j < n ? (int)(tp[p.N - 1 - si[j0 + j]] != 0) : 0;
            hit |= (unsigned)v[j] << j;
        }
        const int total = det_block_scan(v, ipart);
#pragma unroll
        for (int j = 0; j < DET_PER; ++j) {
            if (j0 + j < n) {
                const int inc = M + v[j];
                ctp[j0 + j] = inc;
                if ((hit >> j) & 1u) mpos[inc - 1] = (int)(j0 + j);
            }
        }
        M += total;
    }
    __syncthreads();
    return M;
}

__device__ __forceinline__ void det_no_predictions(const det_p& p, int c, int t, double* md) {
    for (int k = threadIdx.x; k < DET_NE; k += DET_THREADS) {
        md[k] = k == DET_NE - 1 ? 1.0 : (double)k * 0.01;
        md[DET_NE + k] = 0.0;
        md[2 * DET_NE + k] = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) md[(3 + e) * DET_NE + k] = 1.0;
    }
    if (threadIdx.x == 0) {
        p.ap[c * p.T + t] = 0.0;
        if (t == p.tp_index)
            for (int e = 0; e < 4; ++e) p.tp_err[c * 4 + e] = 1.0;
    }
}

__global__ __launch_bounds__(DET_THREADS) void det_curve_kernel(det_p p) {
    __shared__ int ipart[DET_WAVES];
    __shared__ double dpart[DET_WAVES];
    __shared__ double conf_s[DET_NE], prec_s[DET_NE], err_s[4][DET_NE];
    const int c = (int)blockIdx.x / p.T, t = (int)blockIdx.x % p.T;
    double* md = p.md + ((int64_t)c * p.T + t) * 7 * DET_NE;
    const int64_t a = det_lower_bound(p.sk_class, p.N, (int64_t)c << 32);
    const int64_t n = det_lower_bound(p.sk_class, p.N, (int64_t)(c + 1) << 32) - a;
    const int npos = p.npos[c];
    const int64_t* si = p.si_class + a;
    int* ctp = p.ws_ctp + (int64_t)t * p.N + a;
    int* mpos = p.ws_mpos + (int64_t)t * p.N + a;
    double* cm = p.ws_cm + (int64_t)t * p.N + a;
    const unsigned char* tp = p.tp + (int64_t)t * p.N;

    const int M = det_scan_tp(p, tp, si, n, ctp, mpos, ipart);
    if (npos == 0 || M == 0) {
        det_no_predictions(p, c, t, md);
        return;
    }

    const double dn = (double)npos;
    const int64_t last = n - 1;
    auto score_at = [&](int64_t j) { return (double)p.pscore[p.N - 1 - si[j]]; };
    auto rec_at = [&](int64_t j) { return (double)ctp[j] / dn; };
    auto prec_at = [&](int64_t j) { return (double)ctp[j] / (double)(j + 1); };
    if (threadIdx.x < DET_NE) {
        const int k = threadIdx.x;
        const double r = k == DET_NE - 1 ? 1.0 : (double)k * 0.01;
        double pr, cf;
        if (r > rec_at(last)) {
            pr = 0.0, cf = 0.0;
        } else if (r < rec_at(0)) {
            pr = prec_at(0), cf = score_at(0);
        } else {
            int64_t lo = 0, hi = n;   // rec(lo) <= r < rec(hi)
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (rec_at(mid) <= r) lo = mid; else hi = mid;
            }
            const double x0 = rec_at(lo);
            if (lo == last || x0 == r) {
                pr = prec_at(lo), cf = score_at(lo);
            } else {
                const double dxp = rec_at(lo + 1) - x0, dx = r - x0;
                const double sp = (prec_at(lo + 1) - prec_at(lo)) / dxp;
                const double sc = (score_at(lo + 1) - score_at(lo)) / dxp;
                pr = sp * dx + prec_at(lo);
                cf = sc * dx + score_at(lo);
            }
        }
        md[k] = r;
        md[DET_NE + k] = pr;
        md[2 * DET_NE + k] = cf;
        conf_s[k] = cf;
        prec_s[k] = pr;
    }

    auto mscore = [&](int m) { return score_at(mpos[m]); };
    for (int e = 0; e < 4; ++e) {
        const double* err = p.err + ((int64_t)t * 4 + e) * p.N;
        __syncthreads();   // the resampling of the error before has read cm
        double srun = 0.0;
        int crun = 0;
        for (int base = 0; base < M; base += DET_CHUNK) {
            double v[DET_PER];
            int u[DET_PER];
            const int m0 = base + (int)threadIdx.x * DET_PER;
#pragma unroll
            for (int j = 0; j < DET_PER; ++j) {
                double x = 0.0;
                int ok = 0;
                if (m0 + j < M) {
                    x = err[p.N - 1 - si[mpos[m0 + j]]];
                    ok = x == x ? 1 : 0;
                    if (!ok) x = 0.0;
                }
                v[j] = x, u[j] = ok;
            }
            const double vt = det_block_scan(v, dpart);
            const int ut = det_block_scan(u, ipart);
#pragma unroll
            for (int j = 0; j < DET_PER; ++j) {
                if (m0 + j < M) {
                    const int cnt = crun + u[j];
                    cm[m0 + j] = cnt != 0 ? (srun + v[j]) / (double)cnt : 0.0;
                }
            }
            srun = srun + vt;
            crun += ut;
        }
        __syncthreads();
        const bool all_nan = crun == 0;
        if (threadIdx.x < DET_NE) {
            const int k = threadIdx.x;
            const double x = conf_s[k];
            auto cmv = [&](int m) { return all_nan ? 1.0 : cm[m]; };
            double val;
            if (x > mscore(0)) {
                val = cmv(0);
            } else if (x < mscore(M - 1)) {
                val = cmv(M - 1);
            } else {
                int lo = -1, hi = M - 1;   // mscore(hi) <= x < mscore(lo): the smallest m at or below x
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (mscore(mid) <= x) hi = mid; else lo = mid;
                }
                const double x0 = mscore(hi);
                if (hi == 0 || x0 == x) {
                    val = cmv(hi);
                } else {
                    const double slope = (cmv(hi - 1) - cmv(hi)) / (mscore(hi - 1) - x0);
                    val = slope * (x - x0) + cmv(hi);
                }
            }
            md[(3 + e) * DET_NE + k] = val;
            err_s[e][k] = val;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = p.first_ind; k < DET_NE; ++k) {
            const double d = prec_s[k] - p.min_precision;
            s = s + (d > 0.0 ? d : 0.0);
        }
        p.ap[c * p.T + t] = (s / (double)(DET_NE - p.first_ind)) / (1.0 - p.min_precision);
    }
    if (t == p.tp_index && threadIdx.x < 4) {
        const int e = threadIdx.x;
        int lastk = 0;
        for (int k = 0; k < DET_NE; ++k)
            if (conf_s[k] != 0.0) lastk = k;
        double r = 1.0;
        if (lastk >= p.first_ind) {
            double s = 0.0;
            for (int k = p.first_ind; k <= lastk; ++k) s = s + err_s[e][k];
            r = s / (double)(lastk - p.first_ind + 1);
        }
        p.tp_err[c * 4 + e] = r;
    }
}

// ---- interpolated APs ---------------------------------------------------------------------------------
// env[j] = max over k >= j of prec[k] is only read at the matches, and between two matches prec falls (the count
// stays, the position grows), so env[pos(m)] = max over m' >= m of m' / (pos(m') + 1): a reverse running maximum over
// the M matches.  A maximum selects, it does not round: any tree gives the same bits.  It is kept in the workspace
// slot of the curves' cumulative mean.
__global__ __launch_bounds__(DET_THREADS) void det_ap_interp_kernel(det_p p, det_iou_p q) {
    __shared__ int ipart[DET_WAVES];
    __shared__ double dpart[DET_WAVES];
    __shared__ double stage[DET_CHUNK];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = (int)blockIdx.x / p.T, t = (int)blockIdx.x % p.T;
    const int64_t a = det_lower_bound(p.sk_class, p.N, (int64_t)c << 32);
    const int64_t n = det_lower_bound(p.sk_class, p.N, (int64_t)(c + 1) << 32) - a;
    const int npos = p.npos[c];
    int* ctp = p.ws_ctp + (int64_t)t * p.N + a;
    int* mpos = p.ws_mpos + (int64_t)t * p.N + a;
    double* env = p.ws_cm + (int64_t)t * p.N + a;
    double* out = q.ap_interp + ((int64_t)c * p.T + t) * 2;
    const int M = det_scan_tp(p, p.tp + (int64_t)t * p.N, p.si_class + a, n, ctp, mpos, ipart);
    if (npos == 0 || M == 0) {
        if (tid == 0) out[0] = 0.0, out[1] = 0.0;
        return;
    }
    // from the last match backwards: term r is match M - 1 - r, the (M - r)-th
    double carry = 0.0;   // precisions are positive
    for (int base = 0; base < M; base += DET_CHUNK) {
        double v[DET_PER];
        const int r0 = base + tid * DET_PER;
#pragma unroll
        for (int j = 0; j < DET_PER; ++j) {
            const int r = r0 + j;
            v[j] = r < M ? (double)(M - r) / (double)(mpos[M - 1 - r] + 1) : 0.0;
        }
#pragma unroll
        for (int j = 1; j < DET_PER; ++j) v[j] = fmax(v[j - 1], v[j]);
        double run = v[DET_PER - 1];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double o = wave_shfl_up(run, d);
            if (lane >= d) run = fmax(o, run);
        }
        __syncthreads();   // dpart may still be read from the chunk before
        if (lane == 63) dpart[w] = run;
        __syncthreads();
        double before = 0.0, total = 0.0;
#pragma unroll
        for (int k = 0; k < DET_WAVES; ++k) {
            if (k == w) before = total;
            total = fmax(total, dpart[k]);
        }
        double tb = wave_shfl_up(run, 1);
        if (lane == 0) tb = 0.0;
        const double behind = fmax(carry, fmax(before, tb));
#pragma unroll
        for (int j = 0; j < DET_PER; ++j) {
            const int r = r0 + j;
            if (r < M) env[M - 1 - r] = fmax(behind, v[j]);
        }
        carry = fmax(carry, total);
    }
    __syncthreads();
    // the serial sum in match order: one thread adds, all of them stage its terms in LDS
    double s = 0.0;
    for (int base = 0; base < M; base += DET_CHUNK) {
        const int cnt = M - base < DET_CHUNK ? M - base : DET_CHUNK;
        for (int k = tid; k < cnt; k += DET_THREADS) stage[k] = env[base + k];
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < cnt; ++k) s = s + stage[k];
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = s / (double)npos;
        double r40 = 0.0;
        for (int k = 1; k <= 40; ++k) {
            const int64_t m = ((int64_t)k * npos + 39) / 40;   // the smallest m with m * 40 >= k * npos
            r40 = r40 + (m <= (int64_t)M ? env[m - 1] : 0.0);
        }
        out[1] = r40 / 40.0;
    }
}

// ---- entry points -------------------------------------------------------------------------------------

extern "C" int64_t cmt_det_eval_args_size(void) { return (int64_t)sizeof(cmt_det_eval_args); }

static bool det_dims_ok(int64_t N, int64_t G, int S, int C, int T) {
    return N >= 0 && N < ((int64_t)1 << 31) && G >= 0 && G < ((int64_t)1 << 31) && S >= 1 && S <= (1 << 24) && C >= 1 &&
           C <= CMT_DET_MAX_CLASSES && T >= 1 && T <= CMT_DET_MAX_THRESHOLDS;
}

static int64_t det_round8(int64_t v) { return (v + 7) & ~(int64_t)7; }

extern "C" int64_t cmt_det_eval_workspace_bytes(int64_t N, int64_t G, int S, int C, int T) {
    if (!det_dims_ok(N, G, S, C, T)) return -1;
    return (int64_t)T * N * 16 + det_round8(G) + 8;
}

static int det_fill(const cmt_det_eval_args* a, det_p& p, const char* who) {
    const std::string w(who);
    CMT_REQUIRE(a != nullptr, w + ": null argument struct");
    CMT_REQUIRE(a->N >= 0 && a->N < ((int64_t)1 << 31), w + ": N must be in [0, 2^31)");
    CMT_REQUIRE(a->G >= 0 && a->G < ((int64_t)1 << 31), w + ": G must be in [0, 2^31)");
    CMT_REQUIRE(a->S >= 1 && a->S <= (1 << 24), w + ": S must be in [1, 2^24]");
    CMT_REQUIRE(a->C >= 1 && a->C <= CMT_DET_MAX_CLASSES, w + ": C must be in [1, 32]");
    CMT_REQUIRE(a->T >= 1 && a->T <= CMT_DET_MAX_THRESHOLDS, w + ": T must be in [1, 8]");
    CMT_REQUIRE(a->tp_index >= 0 && a->tp_index < a->T, w + ": tp_index must be in [0, T)");
    CMT_REQUIRE(a->first_ind >= 1 && a->first_ind <= 100, w + ": first_ind must be in [1, 100]");
    CMT_REQUIRE(a->min_precision >= 0.0 && a->min_precision < 1.0, w + ": min_precision must be in [0, 1)");
    for (int c = 0; c < a->C; ++c) {
        CMT_REQUIRE(std::isfinite(a->range[c]) && a->range[c] > 0.0, w + ": range must be finite and positive");
        CMT_REQUIRE(std::isfinite(a->yaw_period[c]) && a->yaw_period[c] > 0.0, w + ": yaw_period must be finite and positive");
    }
    for (int t = 0; t < a->T; ++t)
        CMT_REQUIRE(std::isfinite(a->dist_th[t]) && a->dist_th[t] > 0.0, w + ": dist_th must be finite and positive");
    p.N = a->N, p.G = a->G, p.S = a->S, p.C = a->C, p.T = a->T, p.tp_index = a->tp_index, p.first_ind = a->first_ind;
    p.match_blocks = cdiv64((int64_t)a->S * a->C, DET_WAVES);
    for (int c = 0; c < CMT_DET_MAX_CLASSES; ++c) p.range[c] = a->range[c < a->C ? c : 0], p.period[c] = a->yaw_period[c < a->C ? c : 0];
    for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t) p.th[t] = a->dist_th[t < a->T ? t : 0];
    p.min_precision = a->min_precision;
    p.pbox = (const float*)a->pred_box, p.pscore = (const float*)a->pred_score, p.gbox = (const float*)a->gt_box;
    p.plabel = (const int*)a->pred_label, p.psample = (const int*)a->pred_sample;
    p.glabel = (const int*)a->gt_label, p.gsample = (const int*)a->gt_sample, p.gnum = (const int*)a->gt_num_pts;
    p.n_pred = a->n_pred, p.n_gt = a->n_gt;
    p.key_class = (int64_t*)a->key_class, p.key_sample = (int64_t*)a->key_sample, p.key_gt = (int64_t*)a->key_gt;
    p.sk_class = (const int64_t*)a->sk_class, p.si_class = (const int64_t*)a->si_class;
    p.sk_sample = (const int64_t*)a->sk_sample, p.si_sample = (const int64_t*)a->si_sample;
    p.sk_gt = (const int64_t*)a->sk_gt, p.si_gt = (const int64_t*)a->si_gt;
    p.tp = (unsigned char*)a->tp, p.match_gt = (int*)a->match_gt, p.err = (double*)a->err, p.npos = (int*)a->npos;
    p.md = (double*)a->md, p.ap = (double*)a->ap, p.tp_err = (double*)a->tp_err;
    char* ws = (char*)a->workspace;
    const int64_t tn = (int64_t)a->T * a->N;
    p.ws_cm = (double*)ws;
    p.ws_ctp = (int*)(ws + tn * 8);
    p.ws_mpos = (int*)(ws + tn * 12);
    p.ws_taken = (unsigned char*)(ws + tn * 16);
    p.match_iou = nullptr;
    return 0;
}

static int det_iou_fill(const cmt_det_eval_args* a, const cmt_det_iou_args* ia, det_iou_p& q, const char* who) {
    const std::string w(who);
    CMT_REQUIRE(ia != nullptr, w + ": null IoU argument struct");
    CMT_REQUIRE(ia->mode == 0 || ia->mode == 1, w + ": mode must be 0 (BEV) or 1 (3D)");
    CMT_REQUIRE(ia->z_origin == 0.f || ia->z_origin == 0.5f, w + ": z_origin must be 0 or 0.5");
    for (int t = 0; t < a->T; ++t)
        CMT_REQUIRE(std::isfinite(ia->iou_th[t]) && ia->iou_th[t] >= 0.f && ia->iou_th[t] < 1.f, w + ": iou_th must be in [0, 1)");
    for (int t = 0; t < CMT_DET_MAX_THRESHOLDS; ++t) q.th[t] = ia->iou_th[t < a->T ? t : 0];
    q.z_origin = ia->z_origin, q.use_3d = ia->mode;
    q.ap_interp = (double*)ia->ap_interp;
    return 0;
}

#define DET_PTR(field, al, rows)                                                                                     \
    CMT_REQUIRE((rows) == 0 || ptr_aligned(a->field, al), std::string(who) + ": " #field " must be non-null and " #al \
                                                                                 "-byte aligned")

static int det_check_inputs(const cmt_det_eval_args* a, const char* who) {
    DET_PTR(pred_box, 4, a->N); DET_PTR(pred_score, 4, a->N); DET_PTR(pred_label, 4, a->N); DET_PTR(pred_sample, 4, a->N);
    DET_PTR(gt_box, 4, a->G); DET_PTR(gt_label, 4, a->G); DET_PTR(gt_sample, 4, a->G); DET_PTR(gt_num_pts, 4, a->G);
    CMT_REQUIRE(ptr_aligned_or_null(a->n_pred, 4) && ptr_aligned_or_null(a->n_gt, 4),
                std::string(who) + ": n_pred and n_gt must be 4-byte aligned");
    return 0;
}

static int det_check_sorted(const cmt_det_eval_args* a, const char* who) {
    DET_PTR(sk_class, 8, a->N); DET_PTR(si_class, 8, a->N); DET_PTR(sk_sample, 8, a->N); DET_PTR(si_sample, 8, a->N);
    DET_PTR(sk_gt, 8, a->G); DET_PTR(si_gt, 8, a->G);
    DET_PTR(tp, 1, a->N); DET_PTR(match_gt, 4, a->N); DET_PTR(err, 8, a->N); DET_PTR(npos, 4, 1);
    DET_PTR(workspace, 8, 1);
    CMT_REQUIRE(a->workspace_bytes >= cmt_det_eval_workspace_bytes(a->N, a->G, a->S, a->C, a->T),
                std::string(who) + ": workspace below cmt_det_eval_workspace_bytes(N, G, S, C, T)");
    return 0;
}

extern "C" int cmt_det_eval_keys(const cmt_det_eval_args* a, void* stream) {
    const char* who = "cmt_det_eval_keys";
    det_p p;
    if (int rc = det_fill(a, p, who)) return rc;
    if (int rc = det_check_inputs(a, who)) return rc;
    DET_PTR(key_class, 8, a->N); DET_PTR(key_sample, 8, a->N); DET_PTR(key_gt, 8, a->G);
    const int64_t rows = a->N > a->G ? a->N : a->G;
    if (rows > 0) det_keys_kernel<<<dim3((unsigned)cdiv64(rows, DET_THREADS)), DET_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch(who);
}

extern "C" int cmt_det_eval_match(const cmt_det_eval_args* a, void* stream) {
    const char* who = "cmt_det_eval_match";
    det_p p;
    if (int rc = det_fill(a, p, who)) return rc;
    if (int rc = det_check_inputs(a, who)) return rc;
    if (int rc = det_check_sorted(a, who)) return rc;
    const int64_t blocks = p.match_blocks + a->C + DET_FILL_BLOCKS;
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), std::string(who) + ": S * C too large for one launch");
    det_match_kernel<<<dim3((unsigned)blocks), DET_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch(who);
}

extern "C" int64_t cmt_det_iou_args_size(void) { return (int64_t)sizeof(cmt_det_iou_args); }

extern "C" int cmt_det_eval_match_iou(const cmt_det_eval_args* a, const cmt_det_iou_args* ia, void* stream) {
    const char* who = "cmt_det_eval_match_iou";
    det_p p;
    det_iou_p q;
    if (int rc = det_fill(a, p, who)) return rc;
    if (int rc = det_iou_fill(a, ia, q, who)) return rc;
    if (int rc = det_check_inputs(a, who)) return rc;
    if (int rc = det_check_sorted(a, who)) return rc;
    CMT_REQUIRE(ptr_aligned_or_null(ia->match_iou, 4), std::string(who) + ": match_iou must be 4-byte aligned");
    p.match_iou = (float*)ia->match_iou;
    const int64_t blocks = p.match_blocks + a->C + DET_FILL_BLOCKS;
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), std::string(who) + ": S * C too large for one launch");
    det_match_iou_kernel<<<dim3((unsigned)blocks), DET_THREADS, 0, (hipStream_t)stream>>>(p, q);
    return cmt_check_launch(who);
}

extern "C" int cmt_det_eval_ap_interp(const cmt_det_eval_args* a, const cmt_det_iou_args* ia, void* stream) {
    const char* who = "cmt_det_eval_ap_interp";
    det_p p;
    det_iou_p q;
    if (int rc = det_fill(a, p, who)) return rc;
    if (int rc = det_iou_fill(a, ia, q, who)) return rc;
    if (int rc = det_check_inputs(a, who)) return rc;
    if (int rc = det_check_sorted(a, who)) return rc;
    CMT_REQUIRE(ptr_aligned(ia->ap_interp, 8), std::string(who) + ": ap_interp must be non-null and 8-byte aligned");
    det_ap_interp_kernel<<<dim3((unsigned)(a->C * a->T)), DET_THREADS, 0, (hipStream_t)stream>>>(p, q);
    return cmt_check_launch(who);
}

extern "C" int cmt_det_eval_curves(const cmt_det_eval_args* a, void* stream) {
    const char* who = "cmt_det_eval_curves";
    det_p p;
    if (int rc = det_fill(a, p, who)) return rc;
    if (int rc = det_check_inputs(a, who)) return rc;
    if (int rc = det_check_sorted(a, who)) return rc;
    DET_PTR(md, 8, 1); DET_PTR(ap, 8, 1); DET_PTR(tp_err, 8, 1);
    det_curve_kernel<<<dim3((unsigned)(a->C * a->T)), DET_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch(who);
}
