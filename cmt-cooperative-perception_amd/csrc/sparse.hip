// Sparse 3-D convolution for the LiDAR middle encoder (mmdet3d SparseEncoder on spconv):
// a site index (one bit per grid site + running popcounts), the two rulebooks (submanifold
// and strided), the output-stationary bf16x3 MFMA convolution and the scatter to the dense
// BEV map.  Declared in include/cmt_hip.h (cmt_sparse_*).  No call synchronises with the
// host: row counts are read from device memory, grids are sized by capacity.
#include "cmt_common.h"

namespace {

constexpr int SP_HDR = 8;                 // int32 words of header in front of the index (word 0: number of active sites)
constexpr int SP_SCAN_THREADS = 256;
constexpr int SP_SCAN_PER = 16;           // words per thread of the word scan
constexpr int SP_SCAN_SHIFT = 12;         // log2(SP_SCAN_THREADS * SP_SCAN_PER): words per scan block
constexpr int SP_MAX_K = 27;              // taps (3 x 3 x 3)
constexpr int SP_TILE = 128;              // output rows per workgroup of the convolution (4 waves x 32)

// Device view of one index buffer:  [SP_HDR header][bits: words][prefix: words][blockoff: nblocks]
// [rank2row: cap], all 32-bit.  rank(site) = blockoff[word >> 12] + prefix[word] + popcount(bits below).
struct SpIndex {
    int* total;
    unsigned* bits;
    int* prefix;
    int* blockoff;
    int* rank2row;
    int B, D, H, W, words, nblocks, cap;
};

inline int64_t sp_sites(int B, int D, int H, int W) { return (int64_t)B * D * H * W; }

inline int64_t sp_index_bytes(int B, int D, int H, int W, int cap) {
    const int64_t words = (sp_sites(B, D, H, W) + 31) / 32;
    const int64_t nblocks = (words + (1 << SP_SCAN_SHIFT) - 1) >> SP_SCAN_SHIFT;
    const int64_t b = 4 * (SP_HDR + 2 * words + nblocks + (int64_t)cap);
    return (b + 255) / 256 * 256;
}

inline SpIndex sp_view(void* base, int B, int D, int H, int W, int cap) {
    SpIndex ix;
    ix.B = B; ix.D = D; ix.H = H; ix.W = W; ix.cap = cap;
    ix.words = (int)((sp_sites(B, D, H, W) + 31) / 32);
    ix.nblocks = (ix.words + (1 << SP_SCAN_SHIFT) - 1) >> SP_SCAN_SHIFT;
    int* p = (int*)base;
    ix.total = p;
    ix.bits = (unsigned*)(p + SP_HDR);
    ix.prefix = p + SP_HDR + ix.words;
    ix.blockoff = ix.prefix + ix.words;
    ix.rank2row = ix.blockoff + ix.nblocks;
    return ix;
}

__device__ __forceinline__ int sp_count(const int* count, int cap) {
    const int n = *count;
    return n < 0 ? 0 : (n < cap ? n : cap);
}

// the row of site (b, z, y, x), or -1 (inactive, or outside the grid)
__device__ __forceinline__ int sp_lookup(const SpIndex& ix, int b, int z, int y, int x) {
    if ((unsigned)b >= (unsigned)ix.B || (unsigned)z >= (unsigned)ix.D || (unsigned)y >= (unsigned)ix.H ||
        (unsigned)x >= (unsigned)ix.W)
        return -1;
    const int site = ((b * ix.D + z) * ix.H + y) * ix.W + x;
    const int w = site >> 5, bit = site & 31;
    const unsigned u = ix.bits[w];
    if (!((u >> bit) & 1u)) return -1;
    const int rank = ix.blockoff[w >> SP_SCAN_SHIFT] + ix.prefix[w] + __popc(u & ((1u << bit) - 1u));
    return rank < ix.cap ? ix.rank2row[rank] : -1;
}

__global__ void sp_mark_rows(SpIndex ix, const int* coors, const int* count, int n_cap) {
    const int n = sp_count(count, n_cap);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = coors[4 * i], z = coors[4 * i + 1], y = coors[4 * i + 2], x = coors[4 * i + 3];
    if ((unsigned)b >= (unsigned)ix.B || (unsigned)z >= (unsigned)ix.D || (unsigned)y >= (unsigned)ix.H ||
        (unsigned)x >= (unsigned)ix.W)
        return;
    const int site = ((b * ix.D + z) * ix.H + y) * ix.W + x;
    atomicOr(ix.bits + (site >> 5), 1u << (site & 31));
}

// prefix[w] = set bits in the words of w's scan block before w; blockoff[block] = the block's total
__global__ __launch_bounds__(SP_SCAN_THREADS) void sp_scan_words(SpIndex ix) {
    __shared__ int s_sum[SP_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t base = ((int64_t)blockIdx.x << SP_SCAN_SHIFT) + tid * SP_SCAN_PER;
    int pc[SP_SCAN_PER];
    int sum = 0;
#pragma unroll
    for (int j = 0; j < SP_SCAN_PER; ++j) {
        const int64_t w = base + j;
        pc[j] = w < ix.words ? __popc(ix.bits[w]) : 0;
        sum += pc[j];
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < SP_SCAN_THREADS; d <<= 1) {
        const int v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;   // exclusive
#pragma unroll
    for (int j = 0; j < SP_SCAN_PER; ++j) {
        const int64_t w = base + j;
        if (w < ix.words) ix.prefix[w] = run;
        run += pc[j];
    }
    if (tid == SP_SCAN_THREADS - 1) ix.blockoff[blockIdx.x] = s_sum[tid];
}

// exclusive scan of the block totals in place (one workgroup; nblocks <= 2^14), total -> header
__global__ __launch_bounds__(1024) void sp_scan_blocks(SpIndex ix) {
    __shared__ int s_sum[1024];
    const int tid = threadIdx.x;
    const int per = (ix.nblocks + 1023) / 1024;
    const int lo = tid * per;
    int sum = 0;
    for (int j = 0; j < per; ++j)
        if (lo + j < ix.nblocks) sum += ix.blockoff[lo + j];
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int j = 0; j < per; ++j)
        if (lo + j < ix.nblocks) {
            const int v = ix.blockoff[lo + j];
            ix.blockoff[lo + j] = run;
            run += v;
        }
    if (tid == 1023) *ix.total = s_sum[tid];
}

// rank -> row: the lowest row index of a site (rows with equal coordinates: the first one wins)
__global__ void sp_fill_rank2row(SpIndex ix, const int* coors, const int* count, int n_cap) {
    const int n = sp_count(count, n_cap);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = coors[4 * i], z = coors[4 * i + 1], y = coors[4 * i + 2], x = coors[4 * i + 3];
    if ((unsigned)b >= (unsigned)ix.B || (unsigned)z >= (unsigned)ix.D || (unsigned)y >= (unsigned)ix.H ||
        (unsigned)x >= (unsigned)ix.W)
        return;
    const int site = ((b * ix.D + z) * ix.H + y) * ix.W + x;
    const int w = site >> 5, bit = site & 31;
    const unsigned u = ix.bits[w];
    const int rank = ix.blockoff[w >> SP_SCAN_SHIFT] + ix.prefix[w] + __popc(u & ((1u << bit) - 1u));
    if (rank < ix.cap) atomicMin(ix.rank2row + rank, i);
}

struct SpGeom {
    int k[3], s[3], p[3];
    int K;
};

__device__ __forceinline__ void sp_tap(const SpGeom& g, int k, int& kz, int& ky, int& kx) {
    kx = k % g.k[2];
    const int t = k / g.k[2];
    ky = t % g.k[1];
    kz = t / g.k[1];
}

__global__ void sp_nbr_subm(SpIndex ix, SpGeom g, const int* coors, const int* count, int n_cap, int* nbr) {
    const int n = sp_count(count, n_cap);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n_cap * g.K) return;
    const int m = (int)(t / g.K), k = (int)(t % g.K);
    int j = -1;
    if (m < n) {
        int kz, ky, kx;
        sp_tap(g, k, kz, ky, kx);
        j = sp_lookup(ix, coors[4 * m], coors[4 * m + 1] + kz - g.p[0], coors[4 * m + 2] + ky - g.p[1],
                      coors[4 * m + 3] + kx - g.p[2]);
    }
    nbr[t] = j;
}

// every output site whose window holds input row i: o = (i + p - k) / s where that divides
__global__ void sp_mark_down(SpIndex ox, SpGeom g, const int* coors, const int* count, int n_cap, int inB, int inD,
                             int inH, int inW) {
    const int n = sp_count(count, n_cap);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * g.K) return;
    const int i = (int)(t / g.K), k = (int)(t % g.K);
    const int b = coors[4 * i], z = coors[4 * i + 1], y = coors[4 * i + 2], x = coors[4 * i + 3];
    if ((unsigned)b >= (unsigned)inB || (unsigned)z >= (unsigned)inD || (unsigned)y >= (unsigned)inH ||
        (unsigned)x >= (unsigned)inW)
        return;
    int kz, ky, kx;
    sp_tap(g, k, kz, ky, kx);
    const int tz = z + g.p[0] - kz, ty = y + g.p[1] - ky, tx = x + g.p[2] - kx;
    if (tz < 0 || ty < 0 || tx < 0 || tz % g.s[0] || ty % g.s[1] || tx % g.s[2]) return;
    const int oz = tz / g.s[0], oy = ty / g.s[1], oxx = tx / g.s[2];
    if (oz >= ox.D || oy >= ox.H || oxx >= ox.W) return;
    const int site = ((b * ox.D + oz) * ox.H + oy) * ox.W + oxx;
    atomicOr(ox.bits + (site >> 5), 1u << (site & 31));
}

// output coordinates in ascending site order (= ascending (b, z, y, x)); rank2row is the identity
__global__ void sp_emit_down(SpIndex ox, int* out_coors, int* out_count) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w == 0) {
        const int total = *ox.total;
        *out_count = total > ox.cap ? -1 : total;
    }
    if (w >= ox.words) return;
    unsigned u = ox.bits[w];
    int rank = ox.blockoff[w >> SP_SCAN_SHIFT] + ox.prefix[w];
    while (u) {
        const int bit = __ffs(u) - 1;
        u &= u - 1;
        if (rank < ox.cap) {
            int site = (w << 5) + bit;
            const int x = site % ox.W;
            site /= ox.W;
            const int y = site % ox.H;
            site /= ox.H;
            const int z = site % ox.D;
            const int b = site / ox.D;
            out_coors[4 * rank] = b;
            out_coors[4 * rank + 1] = z;
            out_coors[4 * rank + 2] = y;
            out_coors[4 * rank + 3] = x;
            ox.rank2row[rank] = rank;
        }
        ++rank;
    }
}

__global__ void sp_nbr_down(SpIndex ix, SpGeom g, const int* out_coors, const int* out_count, int cap, int* nbr) {
    const int n = sp_count(out_count, cap);   // -1 (gave up) counts as no rows
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)cap * g.K) return;
    const int m = (int)(t / g.K), k = (int)(t % g.K);
    int j = -1;
    if (m < n) {
        int kz, ky, kx;
        sp_tap(g, k, kz, ky, kx);
        j = sp_lookup(ix, out_coors[4 * m], out_coors[4 * m + 1] * g.s[0] - g.p[0] + kz,
                      out_coors[4 * m + 2] * g.s[1] - g.p[1] + ky, out_coors[4 * m + 3] * g.s[2] - g.p[2] + kx);
    }
    nbr[t] = j;
}

// ---- convolution -------------------------------------------------------------------------
// Y[m] = act(scale * sum_k X[nbr[m][k]] W[k] + shift (+ R[m])).  A wave owns 32 output rows x
// all Cout (NB blocks of 32 columns, 16 accumulator registers each); a workgroup is four such
// waves (128 rows) sharing one LDS copy of their nbr rows.  Per tap the wave gathers its rows'
// neighbours straight into the MFMA A layout (lane (r, h): row r, channels 8h .. 8h+7 of a
// 16-channel step), splits them hi = bf16(x), lo = bf16(x - hi), and accumulates
// lo*Whi + hi*Wlo + hi*Whi on v_mfma_f32_32x32x16_bf16 in that fixed order; W's hi/lo
// fragments come pre-arranged per lane (cmt_sparse_pack_bytes).  A tap no row of the wave has a
// neighbour at is skipped (ballot).  No atomics: a row's sum has one order whatever tile it is in.
__device__ __forceinline__ void sp_split8(const float* v, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bf16_t h = (bf16_t)v[j];
        hi[j] = h;
        lo[j] = (bf16_t)(v[j] - (float)h);
    }
}

template <int NB>
__global__ __launch_bounds__(256) void sparse_conv_kernel(cmt_sparse_conv_args a) {
    __shared__ int s_nbr[SP_TILE * SP_MAX_K];
    const int n = sp_count(a.count, a.cap);
    const int K = a.K;
    const int tile0 = blockIdx.x * SP_TILE;
    if (tile0 >= n) return;   // whole workgroup
    {
        const int64_t g0 = (int64_t)tile0 * K, gend = (int64_t)n * K;
        for (int t = threadIdx.x; t < SP_TILE * K; t += 256) s_nbr[t] = g0 + t < gend ? a.nbr[g0 + t] : -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = tile0 + wave * 32;
    if (row0 >= n) return;    // wave-uniform, after the only barrier
    const int r = lane & 31, h = lane >> 5;
    const int KC = (a.Cin + 15) >> 4;
    const bool vec = (a.Cin & 7) == 0 && (a.ldx & 3) == 0 && (((uintptr_t)a.X) & 15) == 0;
    const bf16x8* wp = (const bf16x8*)a.Wp;
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

    for (int k = 0; k < K; ++k) {
        int j = s_nbr[(wave * 32 + r) * K + k];
        if ((unsigned)j >= (unsigned)a.n_in_cap) j = -1;
        if (__ballot(j >= 0) == 0) continue;
        const float* xr = a.X + (int64_t)(j < 0 ? 0 : j) * a.ldx;
        for (int kc = 0; kc < KC; ++kc) {
            const int c0 = kc * 16 + 8 * h;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.f;
            if (j >= 0) {
                if (vec && c0 + 8 <= a.Cin) {
                    const f32x4 v0 = *(const f32x4*)(xr + c0), v1 = *(const f32x4*)(xr + c0 + 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v[i] = v0[i];
                        v[4 + i] = v1[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (c0 + i < a.Cin) v[i] = xr[c0 + i];
                }
            }
            bf16x8 ahi, alo;
            sp_split8(v, ahi, alo);
            const bf16x8* wb = wp + ((int64_t)(k * KC + kc) * NB) * 128 + lane;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const bf16x8 bhi = wb[nb * 128], blo = wb[nb * 128 + 64];
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, acc[nb], 0, 0, 0);
            }
        }
    }
    // C/D layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int col = nb * 32 + r;
        if (col >= a.Cout) continue;
        const float sc = a.scale[col], sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (row >= n) continue;
            float y = fmaf(acc[nb][i], sc, sh);
            if (a.R) y += a.R[(int64_t)row * a.ldr + col];
            if (a.relu) y = fmaxf(y, 0.f);
            a.Y[(int64_t)row * a.ldy + col] = y;
        }
    }
}

__global__ void sp_to_dense(cmt_sparse_dense_args a) {
    const int n = sp_count(a.count, a.n_cap);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * a.C) return;
    const int m = (int)(t / a.C), c = (int)(t % a.C);
    const int b = a.coors[4 * m], z = a.coors[4 * m + 1], y = a.coors[4 * m + 2], x = a.coors[4 * m + 3];
    if ((unsigned)b >= (unsigned)a.B || (unsigned)z >= (unsigned)a.D || (unsigned)y >= (unsigned)a.H ||
        (unsigned)x >= (unsigned)a.W)
        return;
    // [B, C, D, H, W] viewed as [B, C * D, H, W]
    a.out[((((int64_t)b * a.C + c) * a.D + z) * a.H + y) * a.W + x] = a.X[(int64_t)m * a.ldx + c];
}

int sp_check_grid(const char* who, int B, int D, int H, int W) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return cmt_fail(CMT_EINVAL, std::string(who) + ": grid extents must be positive");
    if ((double)B * D * H * W >= 2147483648.0 || sp_sites(B, D, H, W) >= ((int64_t)1 << 31))
        return cmt_fail(CMT_EINVAL, std::string(who) + ": grid of B*D*H*W >= 2^31 sites (32-bit site numbers)");
    return CMT_OK;
}

// bits -> prefix / blockoff / total (after the bits are marked)
void sp_scan(const SpIndex& ix, hipStream_t s) {
    sp_scan_words<<<ix.nblocks, SP_SCAN_THREADS, 0, s>>>(ix);
    sp_scan_blocks<<<1, 1024, 0, s>>>(ix);
}

int sp_clear(const SpIndex& ix, const char* who, hipStream_t s) {
    hipError_t e = hipMemsetAsync(ix.total, 0, 4 * ((size_t)SP_HDR + ix.words), s);
    if (e == hipSuccess) e = hipMemsetAsync(ix.rank2row, 0x7f, 4 * (size_t)ix.cap, s);
    if (e != hipSuccess) return cmt_fail((int)e, std::string(who) + ": hipMemsetAsync failed");
    return CMT_OK;
}

int sp_check_geom(const char* who, const cmt_sparse_rulebook_args* a, SpGeom& g) {
    int K = 1;
    for (int i = 0; i < 3; ++i) {
        g.k[i] = a->kernel3[i];
        g.s[i] = a->stride3[i];
        g.p[i] = a->padding3[i];
        if (g.k[i] < 1 || g.k[i] > 3 || g.s[i] < 1 || g.p[i] < 0)
            return cmt_fail(CMT_EINVAL, std::string(who) + ": kernel3 in 1..3, stride3 >= 1 and padding3 >= 0 required");
        K *= g.k[i];
    }
    if (a->K != K) return cmt_fail(CMT_EINVAL, std::string(who) + ": K does not match kernel3 (kD*kH*kW)");
    g.K = K;
    return CMT_OK;
}

}  // namespace

extern "C" int64_t cmt_sparse_index_args_size(void) { return (int64_t)sizeof(cmt_sparse_index_args); }
extern "C" int64_t cmt_sparse_rulebook_args_size(void) { return (int64_t)sizeof(cmt_sparse_rulebook_args); }
extern "C" int64_t cmt_sparse_conv_args_size(void) { return (int64_t)sizeof(cmt_sparse_conv_args); }
extern "C" int64_t cmt_sparse_dense_args_size(void) { return (int64_t)sizeof(cmt_sparse_dense_args); }

extern "C" int64_t cmt_sparse_index_bytes(int B, int D, int H, int W, int cap) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || cap <= 0 || sp_sites(B, D, H, W) >= ((int64_t)1 << 31)) return 0;
    return sp_index_bytes(B, D, H, W, cap);
}

extern "C" int64_t cmt_sparse_pack_bytes(int K, int Cin, int Cout) {
    if (K <= 0 || Cin <= 0 || Cout <= 0) return 0;
    return (int64_t)K * ((Cin + 15) / 16) * ((Cout + 31) / 32) * 2 * 64 * 8 * 2;
}

extern "C" int cmt_sparse_index(const cmt_sparse_index_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_sparse_index: null argument struct");
    CMT_REQUIRE(a->coors && a->count && a->index, "cmt_sparse_index: coors, count and index must be non-null");
    if (int rc = sp_check_grid("cmt_sparse_index", a->B, a->D, a->H, a->W)) return rc;
    CMT_REQUIRE(a->n_cap > 0, "cmt_sparse_index: n_cap must be positive");
    if (a->index_bytes < sp_index_bytes(a->B, a->D, a->H, a->W, a->n_cap))
        return cmt_fail(CMT_EWORKSPACE, "cmt_sparse_index: index buffer too small (cmt_sparse_index_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const SpIndex ix = sp_view(a->index, a->B, a->D, a->H, a->W, a->n_cap);
    if (int rc = sp_clear(ix, "cmt_sparse_index", s)) return rc;
    const int rb = cdiv(a->n_cap, 256);
    sp_mark_rows<<<rb, 256, 0, s>>>(ix, a->coors, a->count, a->n_cap);
    sp_scan(ix, s);
    sp_fill_rank2row<<<rb, 256, 0, s>>>(ix, a->coors, a->count, a->n_cap);
    return cmt_check_launch("cmt_sparse_index");
}

extern "C" int cmt_sparse_rulebook_subm(const cmt_sparse_rulebook_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_sparse_rulebook_subm: null argument struct");
    CMT_REQUIRE(a->coors && a->count && a->index && a->nbr,
                "cmt_sparse_rulebook_subm: coors, count, index and nbr must be non-null");
    if (int rc = sp_check_grid("cmt_sparse_rulebook_subm", a->B, a->D, a->H, a->W)) return rc;
    SpGeom g;
    if (int rc = sp_check_geom("cmt_sparse_rulebook_subm", a, g)) return rc;
    for (int i = 0; i < 3; ++i)
        CMT_REQUIRE((g.k[i] & 1) && g.s[i] == 1 && g.p[i] == g.k[i] / 2,
                    "cmt_sparse_rulebook_subm: odd kernel3, stride3 1 and padding3 = kernel3 / 2 required");
    CMT_REQUIRE(a->n_cap > 0, "cmt_sparse_rulebook_subm: n_cap must be positive");
    if (a->index_bytes < sp_index_bytes(a->B, a->D, a->H, a->W, a->n_cap))
        return cmt_fail(CMT_EWORKSPACE, "cmt_sparse_rulebook_subm: index buffer too small (cmt_sparse_index_bytes)");
    const SpIndex ix = sp_view(const_cast<void*>(a->index), a->B, a->D, a->H, a->W, a->n_cap);
    const int64_t total = (int64_t)a->n_cap * g.K;
    sp_nbr_subm<<<(unsigned)cdiv64(total, 256), 256, 0, (hipStream_t)stream>>>(ix, g, a->coors, a->count, a->n_cap, a->nbr);
    return cmt_check_launch("cmt_sparse_rulebook_subm");
}

extern "C" int cmt_sparse_rulebook_down(const cmt_sparse_rulebook_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_sparse_rulebook_down: null argument struct");
    CMT_REQUIRE(a->coors && a->count && a->index && a->nbr && a->out_index && a->out_coors && a->out_count,
                "cmt_sparse_rulebook_down: coors, count, index, out_index, out_coors, out_count and nbr must be non-null");
    if (int rc = sp_check_grid("cmt_sparse_rulebook_down", a->B, a->D, a->H, a->W)) return rc;
    SpGeom g;
    if (int rc = sp_check_geom("cmt_sparse_rulebook_down", a, g)) return rc;
    CMT_REQUIRE(a->n_cap > 0 && a->cap > 0, "cmt_sparse_rulebook_down: n_cap and cap must be positive");
    const int in3[3] = {a->D, a->H, a->W};
    int out3[3];
    for (int i = 0; i < 3; ++i) {
        CMT_REQUIRE(in3[i] + 2 * g.p[i] >= g.k[i], "cmt_sparse_rulebook_down: kernel larger than the padded grid");
        out3[i] = (in3[i] + 2 * g.p[i] - g.k[i]) / g.s[i] + 1;
    }
    if (a->index_bytes < sp_index_bytes(a->B, a->D, a->H, a->W, a->n_cap) ||
        a->out_index_bytes < sp_index_bytes(a->B, out3[0], out3[1], out3[2], a->cap))
        return cmt_fail(CMT_EWORKSPACE, "cmt_sparse_rulebook_down: index or out_index too small (cmt_sparse_index_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const SpIndex ix = sp_view(const_cast<void*>(a->index), a->B, a->D, a->H, a->W, a->n_cap);
    const SpIndex ox = sp_view(a->out_index, a->B, out3[0], out3[1], out3[2], a->cap);
    if (int rc = sp_clear(ox, "cmt_sparse_rulebook_down", s)) return rc;
    sp_mark_down<<<(unsigned)cdiv64((int64_t)a->n_cap * g.K, 256), 256, 0, s>>>(ox, g, a->coors, a->count, a->n_cap, a->B,
                                                                                 a->D, a->H, a->W);
    sp_scan(ox, s);
    sp_emit_down<<<cdiv(ox.words, 256), 256, 0, s>>>(ox, a->out_coors, a->out_count);
    sp_nbr_down<<<(unsigned)cdiv64((int64_t)a->cap * g.K, 256), 256, 0, s>>>(ix, g, a->out_coors, a->out_count, a->cap,
                                                                              a->nbr);
    return cmt_check_launch("cmt_sparse_rulebook_down");
}

extern "C" int cmt_sparse_conv(const cmt_sparse_conv_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_sparse_conv: null argument struct");
    CMT_REQUIRE(a->X && a->nbr && a->count && a->Wp && a->scale && a->shift && a->Y,
                "cmt_sparse_conv: X, nbr, count, Wp, scale, shift and Y must be non-null");
    CMT_REQUIRE(a->Cout >= 1 && a->Cout <= 128, "cmt_sparse_conv: Cout must be in 1..128");
    CMT_REQUIRE(a->Cin >= 1 && a->Cin <= 128, "cmt_sparse_conv: Cin must be in 1..128");
    CMT_REQUIRE(a->K >= 1 && a->K <= SP_MAX_K, "cmt_sparse_conv: K must be in 1..27");
    CMT_REQUIRE(a->cap > 0 && a->n_in_cap > 0, "cmt_sparse_conv: cap and n_in_cap must be positive");
    CMT_REQUIRE(a->ldx >= a->Cin && a->ldy >= a->Cout && (!a->R || a->ldr >= a->Cout),
                "cmt_sparse_conv: ldx < Cin, ldy < Cout or ldr < Cout");
    CMT_REQUIRE(a->wp_bytes == cmt_sparse_pack_bytes(a->K, a->Cin, a->Cout),
                "cmt_sparse_conv: wp_bytes is not cmt_sparse_pack_bytes(K, Cin, Cout)");
    CMT_REQUIRE((((uintptr_t)a->Wp) & 15) == 0, "cmt_sparse_conv: Wp must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int grid = cdiv(a->cap, SP_TILE);
    switch ((a->Cout + 31) / 32) {
        case 1: sparse_conv_kernel<1><<<grid, 256, 0, s>>>(*a); break;
        case 2: sparse_conv_kernel<2><<<grid, 256, 0, s>>>(*a); break;
        case 3: sparse_conv_kernel<3><<<grid, 256, 0, s>>>(*a); break;
        default: sparse_conv_kernel<4><<<grid, 256, 0, s>>>(*a); break;
    }
    return cmt_check_launch("cmt_sparse_conv");
}

extern "C" int cmt_sparse_to_dense(const cmt_sparse_dense_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_sparse_to_dense: null argument struct");
    CMT_REQUIRE(a->X && a->coors && a->count && a->out, "cmt_sparse_to_dense: X, coors, count and out must be non-null");
    if (int rc = sp_check_grid("cmt_sparse_to_dense", a->B, a->D, a->H, a->W)) return rc;
    CMT_REQUIRE(a->C > 0 && a->n_cap > 0 && a->ldx >= a->C, "cmt_sparse_to_dense: C and n_cap must be positive, ldx >= C");
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = sizeof(float) * (size_t)sp_sites(a->B, a->D, a->H, a->W) * (size_t)a->C;
    if (hipMemsetAsync(a->out, 0, bytes, s) != hipSuccess) return cmt_fail(CMT_EINVAL, "cmt_sparse_to_dense: hipMemsetAsync failed");
    sp_to_dense<<<(unsigned)cdiv64((int64_t)a->n_cap * a->C, 256), 256, 0, s>>>(*a);
    return cmt_check_launch("cmt_sparse_to_dense");
}
