// cmt_lsap: batched rectangular linear sum assignment on the device (the
// scipy.optimize.linear_sum_assignment call of HungarianAssigner3D,
// hungarian_assigner_3d.py:139-147), see include/cmt_hip.h.
//
// Two launches after a memset of status[]:
//   lsap_prep_kernel   per problem: the cost matrix into the workspace with the
//                      SMALLER side as rows ([nr][nc] row-major: a 32x32 LDS
//                      tile transpose when ngt <= Nq, a copy otherwise), and the
//                      finiteness check (status |= 1).
//   lsap_solve_kernel  one wave per problem: the shortest augmenting path
//                      method of scipy's rectangular_lsap (Crouse's JV variant)
//                      in float64.  Lane l owns columns l, l + 64, ...: their
//                      path cost, dual v and done bit stay in registers; the
//                      row duals, both matchings, the path back-pointers and the
//                      rows visited by the current search sit in LDS.  One
//                      column is finalised per inner step (a wave argmin over
//                      (value, index) pairs, ties to the lowest index), so the
//                      loops are bounded by nr augmentations of at most nc
//                      steps whatever the data holds.
#include "cmt_common.h"

namespace {

constexpr int LSAP_MAX_COLS = 2048;   // max(Nq, ngt)
constexpr int LSAP_MAX_ROWS = 512;    // min(Nq, ngt)
constexpr int LSAP_TILE = 32;

struct lsap_desc {
    int64_t off, ld;
    int Nq, ngt;
    bool ok;
};

// A descriptor the kernels may follow: inside the declared maxima, the solver's limits and the
// cost buffer.  Anything else is answered with status 2 and never dereferenced.
__device__ __forceinline__ lsap_desc lsap_read_desc(const cmt_lsap_args& a, int p) {
    const int64_t* d = a.desc + 4 * (int64_t)p;
    const int64_t off = d[0], nq = d[1], ng = d[2], ld = d[3];
    lsap_desc r;
    r.ok = nq >= 0 && ng >= 0 && nq <= a.max_nq && ng <= a.max_ngt && (nq < ng ? nq : ng) <= LSAP_MAX_ROWS;
    if (r.ok && nq > 0 && ng > 0)
        r.ok = off >= 0 && ld >= ng && off <= a.cost_elems && ld <= a.cost_elems &&
               off + (nq - 1) * ld + ng <= a.cost_elems;
    r.off = off;
    r.ld = ld;
    r.Nq = (int)(nq < 0 ? 0 : (nq > a.max_nq ? a.max_nq : nq));      // clamped: the -1 fill of a refused problem
    r.ngt = (int)(ng < 0 ? 0 : (ng > a.max_ngt ? a.max_ngt : ng));   // stays inside its own output rows
    return r;
}

__device__ __forceinline__ bool lsap_nonfinite(float x) {
    return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// grid (tiles of the largest problem, P), 256 threads: 32 x 8
__global__ __launch_bounds__(256) void lsap_prep_kernel(cmt_lsap_args a) {
    const int p = blockIdx.y;
    const lsap_desc d = lsap_read_desc(a, p);
    if (!d.ok) return;
    const int tg = (a.max_ngt + LSAP_TILE - 1) / LSAP_TILE;
    const int q0 = (blockIdx.x / tg) * LSAP_TILE, g0 = (blockIdx.x % tg) * LSAP_TILE;
    if (q0 >= d.Nq || g0 >= d.ngt) return;
    __shared__ float tile[LSAP_TILE][LSAP_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* src = a.cost + d.off;
    float* ws = (float*)a.workspace + (int64_t)p * a.max_nq * a.max_ngt;
    const bool tr = d.ngt <= d.Nq;   // rows of the workspace copy = GTs
    bool bad = false;
    for (int r = ty; r < LSAP_TILE; r += 8) {
        const int q = q0 + r, g = g0 + tx;
        if (q < d.Nq && g < d.ngt) {
            const float x = src[(int64_t)q * d.ld + g];
            bad |= lsap_nonfinite(x);
            if (tr) tile[r][tx] = x;
            else ws[(int64_t)q * d.ngt + g] = x;
        }
    }
    if (tr) {
        __syncthreads();
        for (int r = ty; r < LSAP_TILE; r += 8) {
            const int g = g0 + r, q = q0 + tx;
            if (q < d.Nq && g < d.ngt) ws[(int64_t)g * d.Nq + q] = tile[tx][r];
        }
    }
    if (bad) atomicOr(a.status + p, 1);
}

// ---- wave argmin over (path cost, column) pairs, ties to the lowest column ----------------------
// No LDS round trip (a __shfl_xor butterfly is 18 dependent ds_bpermute per step): lanes ^1 and ^2
// by DPP quad_perm, then the mirrored half row and row (after the quad stages every quad is
// uniform, so reading lane 7 - i / 15 - i reaches the other quad / half row), then the 16- and
// 32-lane row swaps of gfx950.  Every lane ends with the wave's minimum.
struct lsap_cand {
    double v;
    int j;
};

__device__ __forceinline__ lsap_cand lsap_min(lsap_cand a, lsap_cand b) {
    return (b.v < a.v || (b.v == a.v && b.j < a.j)) ? b : a;
}

template <int CTRL>
__device__ __forceinline__ lsap_cand lsap_dpp(lsap_cand c) {
    lsap_cand o;
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(c.v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(c.v), CTRL, 0xf, 0xf, true);
    o.v = __hiloint2double(hi, lo);
    o.j = __builtin_amdgcn_update_dpp(0, c.j, CTRL, 0xf, 0xf, true);
    return o;
}

template <bool ROWS32>
__device__ __forceinline__ lsap_cand lsap_swap_min(lsap_cand c) {
    const unsigned lo = (unsigned)__double2loint(c.v), hi = (unsigned)__double2hiint(c.v), j = (unsigned)c.j;
    lsap_cand a, b;
    if (ROWS32) {
        const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        const auto rj = __builtin_amdgcn_permlane32_swap(j, j, false, false);
        a.v = __hiloint2double((int)rh[0], (int)rl[0]);
        b.v = __hiloint2double((int)rh[1], (int)rl[1]);
        a.j = (int)rj[0];
        b.j = (int)rj[1];
    } else {
        const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const auto rj = __builtin_amdgcn_permlane16_swap(j, j, false, false);
        a.v = __hiloint2double((int)rh[0], (int)rl[0]);
        b.v = __hiloint2double((int)rh[1], (int)rl[1]);
        a.j = (int)rj[0];
        b.j = (int)rj[1];
    }
    return lsap_min(a, b);
}

__device__ __forceinline__ lsap_cand lsap_wave_argmin(lsap_cand c) {
    c = lsap_min(c, lsap_dpp<0xb1>(c));    // quad_perm [1, 0, 3, 2]
    c = lsap_min(c, lsap_dpp<0x4e>(c));    // quad_perm [2, 3, 0, 1]
    c = lsap_min(c, lsap_dpp<0x141>(c));   // row_half_mirror
    c = lsap_min(c, lsap_dpp<0x140>(c));   // row_mirror
    c = lsap_swap_min<false>(c);           // rows 0 <-> 1, 2 <-> 3
    return lsap_swap_min<true>(c);         // lanes 0-31 <-> 32-63
}

__device__ __forceinline__ void lsap_fill(int* dst, int n, int lane) {
    if (dst)
        for (int i = lane; i < n; i += 64) dst[i] = -1;
}

// grid P, one wave each; CPL = columns per lane (the host picks it from max(max_nq, max_ngt))
template <int CPL>
__global__ __launch_bounds__(64) void lsap_solve_kernel(cmt_lsap_args a) {
    constexpr int NCOL = CPL * 64;
    __shared__ int s_path[NCOL];              // column -> the row its shortest path comes from
    __shared__ int s_row4col[NCOL];           // column -> matched row or -1
    __shared__ int s_col4row[LSAP_MAX_ROWS];  // row -> matched column or -1
    __shared__ int s_vrow[LSAP_MAX_ROWS];     // rows the current search entered, in order,
    __shared__ double s_vval[LSAP_MAX_ROWS];  // and the path cost of the column each was entered through
    __shared__ double s_u[LSAP_MAX_ROWS];     // row duals

    const int p = blockIdx.x, lane = threadIdx.x;
    const lsap_desc d = lsap_read_desc(a, p);
    int* mq = a.match_q + (int64_t)p * a.ld_q;
    int* mg = a.match_g ? a.match_g + (int64_t)p * a.ld_g : nullptr;
    const int st = d.ok ? a.status[p] : 2;
    const bool tr = d.ngt <= d.Nq;
    const int nr = tr ? d.ngt : d.Nq, nc = tr ? d.Nq : d.ngt;
    if (st != 0 || nr == 0 || nc > NCOL) {    // (nc > NCOL: a launch that does not fit its own maxima)
        lsap_fill(mq, d.ngt, lane);
        lsap_fill(mg, d.Nq, lane);
        if (lane == 0) a.status[p] = st != 0 ? st : (nr == 0 ? 0 : 2);
        return;
    }
    const float* C = (const float*)a.workspace + (int64_t)p * a.max_nq * a.max_ngt;   // [nr][nc]

    double sh[CPL], v[CPL];
    unsigned pad = 0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int j = k * 64 + lane;
        v[k] = 0.0;
        if (j >= nc) pad |= 1u << k;
        s_row4col[j] = -1;
    }
    for (int i = lane; i < nr; i += 64) {
        s_u[i] = 0.0;
        s_col4row[i] = -1;
    }
    __syncthreads();

    const double INF = __builtin_huge_val();
    bool failed = false;
    for (int cur = 0; cur < nr; ++cur) {
        unsigned done = pad;
#pragma unroll
        for (int k = 0; k < CPL; ++k) sh[k] = INF;
        double minVal = 0.0;
        int i = cur, sink = -1, nvis = 0;
        for (int step = 0; step < nc; ++step) {
            const double ui = s_u[i];
            const float* row = C + (int64_t)i * nc;
            float c[CPL];
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int j = k * 64 + lane;
                c[k] = row[j < nc ? j : nc - 1];
            }
            double best = INF;
            int bj = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                if (!((done >> k) & 1u)) {
                    const int j = k * 64 + lane;
                    const double r = ((minVal + (double)c[k]) - ui) - v[k];   // scipy's evaluation order
                    if (r < sh[k]) {
                        sh[k] = r;
                        s_path[j] = i;
                    }
                    if (sh[k] < best) {    // k ascending: the lowest index among this lane's equals
                        best = sh[k];
                        bj = j;
                    }
                }
            }
            const lsap_cand w = lsap_wave_argmin(lsap_cand{best, bj});
            best = w.v;
            bj = w.j;
            if (bj >= nc) break;          // no finite candidate: cannot happen with finite costs
            minVal = best;
            if (lane == (bj & 63)) done |= 1u << (bj >> 6);
            const int r4 = s_row4col[bj];
            if (r4 < 0) {
                sink = bj;
                break;
            }
            if (lane == 0) {
                s_vrow[nvis] = r4;
                s_vval[nvis] = best;
            }
            ++nvis;
            i = r4;
        }
        if (sink < 0) {
            failed = true;
            break;
        }
        __syncthreads();   // s_path, s_vrow, s_vval
        // dual update (scipy: u[cur] += minVal; u[i] += minVal - spc[col4row[i]] for the visited
        // rows -- that path cost is the value their column was selected with; v[j] -= minVal - spc[j])
        if (lane == 0) s_u[cur] += minVal;
        for (int t = lane; t < nvis; t += 64) s_u[s_vrow[t]] += minVal - s_vval[t];
        const unsigned sc = done & ~pad;
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if ((sc >> k) & 1u) v[k] -= minVal - sh[k];
        // augment along the back-pointers: at most nvis + 1 <= nr links
        if (lane == 0) {
            int j = sink;
            for (int t = 0; t <= nvis; ++t) {
                const int r = s_path[j];
                s_row4col[j] = r;
                const int jn = s_col4row[r];
                s_col4row[r] = j;
                j = jn;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (failed) {
        lsap_fill(mq, d.ngt, lane);
        lsap_fill(mg, d.Nq, lane);
        if (lane == 0) a.status[p] = 1;
        return;
    }
    int* of_row = tr ? mq : mg;   // rows are GTs when tr, queries otherwise
    int* of_col = tr ? mg : mq;
    if (of_row)
        for (int i = lane; i < nr; i += 64) of_row[i] = s_col4row[i];
    if (of_col)
        for (int j = lane; j < nc; j += 64) of_col[j] = s_row4col[j];
}

}  // namespace

extern "C" int64_t cmt_lsap_args_size(void) { return (int64_t)sizeof(cmt_lsap_args); }

extern "C" int64_t cmt_lsap_workspace_bytes(int P, int max_nq, int max_ngt) {
    if (P <= 0 || max_nq <= 0 || max_ngt <= 0) return 0;
    const int64_t b = (int64_t)P * max_nq * max_ngt * (int64_t)sizeof(float);
    return (b + 255) / 256 * 256;
}

extern "C" int cmt_lsap(const cmt_lsap_args* ap, void* stream) {
    CMT_REQUIRE(ap != nullptr, "cmt_lsap: null argument struct");
    CMT_REQUIRE(ap->P > 0, "cmt_lsap: P must be positive");
    CMT_REQUIRE(ap->cost && ap->desc && ap->match_q && ap->status && ap->workspace,
                "cmt_lsap: cost, desc, match_q, status and workspace must be non-null");
    CMT_REQUIRE(ap->max_nq > 0 && ap->max_ngt > 0 && ap->cost_elems > 0, "cmt_lsap: max_nq, max_ngt and cost_elems must be positive");
    CMT_REQUIRE(ap->ld_q >= ap->max_ngt && (!ap->match_g || ap->ld_g >= ap->max_nq),
                "cmt_lsap: ld_q < max_ngt or ld_g < max_nq");
    const int hi = ap->max_nq > ap->max_ngt ? ap->max_nq : ap->max_ngt;
    const int lo = ap->max_nq > ap->max_ngt ? ap->max_ngt : ap->max_nq;
    if (hi > LSAP_MAX_COLS || lo > LSAP_MAX_ROWS)
        return cmt_fail(CMT_ENOTSUP, "cmt_lsap: supports max(Nq, ngt) <= 2048 and min(Nq, ngt) <= 512");
    if (ap->P > 65535) return cmt_fail(CMT_ENOTSUP, "cmt_lsap: at most 65535 problems per call");
    if (ap->workspace_bytes < cmt_lsap_workspace_bytes(ap->P, ap->max_nq, ap->max_ngt))
        return cmt_fail(CMT_EWORKSPACE, "cmt_lsap: workspace too small (cmt_lsap_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ap->status, 0, sizeof(int) * (size_t)ap->P, s);
    if (e != hipSuccess) return cmt_fail((int)e, "cmt_lsap: hipMemsetAsync failed");
    const int tiles = ((ap->max_nq + LSAP_TILE - 1) / LSAP_TILE) * ((ap->max_ngt + LSAP_TILE - 1) / LSAP_TILE);
    lsap_prep_kernel<<<dim3(tiles, ap->P), 256, 0, s>>>(*ap);
    if (hi <= 64) lsap_solve_kernel<1><<<ap->P, 64, 0, s>>>(*ap);
    else if (hi <= 128) lsap_solve_kernel<2><<<ap->P, 64, 0, s>>>(*ap);
    else if (hi <= 256) lsap_solve_kernel<4><<<ap->P, 64, 0, s>>>(*ap);
    else if (hi <= 512) lsap_solve_kernel<8><<<ap->P, 64, 0, s>>>(*ap);
    else if (hi <= 1024) lsap_solve_kernel<16><<<ap->P, 64, 0, s>>>(*ap);
    else lsap_solve_kernel<32><<<ap->P, 64, 0, s>>>(*ap);
    return cmt_check_launch("cmt_lsap");
}
