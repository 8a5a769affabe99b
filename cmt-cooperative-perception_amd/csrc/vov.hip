// Image backbone kernels (VoVNet-eSE, the reference's img_backbone), declared in include/cmt_hip.h
// (cmt_img_*):
//   img_stem_kernel      3 x 3 / stride 2 / pad 1 conv from the fp32 NCHW image to CMT_F16P rows
//   img_conv3x3_kernel   3 x 3 / pad 1 conv of stride 1 or 2, pair rows to pair rows, any Cout % 32 <= 256
//   img_concat_kernel    1 x 1 conv over up to 8 pair-row sources (the OSA aggregation without a
//                        concatenated map), with the eSE pool's per-tile column sums
//   img_gate_kernel      eSE gate: hsigmoid(fc(mean)) from the per-tile sums, fp32 FMA
//   img_apply_kernel     x * gate (+ identity) on pair rows
//   img_pool_kernel      3 x 3 / stride 2 / ceil-mode / no-pad max on pair rows
// The conv and the concat are output-stationary: a wave owns 32 output rows x all of the workgroup's
// columns (NB accumulators of 32 columns), gathers an A fragment once per 16-channel step straight
// into the MFMA operand layout (lane (r, h): row r, channels 8h .. 8h+7) and uses it for every column
// block.  W goes through LDS in chunks of 32 k, staged once for the four waves, double-buffered, one
// barrier per chunk.  Three f16 MFMA passes lo*Whi + hi*Wlo + hi*Whi per step with fp32 accumulation
// in fixed K order.  No atomics on the data path (one writer per element), no call synchronises with
// the host.  The second half of the file holds the opt-in one-pass fp16 policy of the same launches
// (cmt_img_*_f16: plain fp16 rows, one MFMA per step).
#include "cmt_common.h"

namespace {

constexpr int IMG_TM = 128;     // output rows per workgroup (4 waves x 32)
constexpr int IMG_KC = 32;      // k per staged chunk of W (two 16-k steps)
constexpr int IMG_WROW = 64;    // 16-bit words per LDS row of a W chunk (hi 32 | lo 32)
constexpr int IMG_CAT_NB = 4;   // concat: 32-column blocks per workgroup (128 output channels)
constexpr int IMG_GATE_OB = 16; // gate: outputs per workgroup (4 per wave)

__device__ __forceinline__ f32x16 mma3(pair8_t ahi, pair8_t alo, pair8_t bhi, pair8_t blo, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, c, 0, 0, 0);
}

// C/D layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__device__ __forceinline__ pair8_t zero8() {
    pair8_t z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (pair_t)0.f;
    return z;
}

// A W chunk: rows [n0, n0 + 32 NB) x (hi | lo) x 32 k from k offset kb of the [N][2][Ktot] pair image.
// Piece i of thread t: row (t >> 3) + 32 i, 16 bytes sub = t & 7 of the row's 128 (hi: sub < 4).  In LDS
// the piece index is XORed with (row >> 1) % 8: two rows fill one 256-byte bank row, so 16 consecutive
// rows at one logical piece (a ds_read_b128 group) fall on 16 distinct 16-byte slots.
template <int NB>
__device__ __forceinline__ void w_load(pair8_t (&q)[NB], const pair_t* Wt, int64_t ldw, int Ktot, int n0, int kb, int t) {
    const int sub = t & 7;
    const pair_t* src = Wt + (int64_t)(n0 + (t >> 3)) * ldw + (sub >> 2) * Ktot + kb + 8 * (sub & 3);
#pragma unroll
    for (int i = 0; i < NB; ++i) q[i] = *(const pair8_t*)(src + (int64_t)(32 * i) * ldw);
}

template <int NB>
__device__ __forceinline__ void w_store(pair_t* buf, const pair8_t (&q)[NB], int t) {
    const int row = t >> 3;
    pair_t* dst = buf + row * IMG_WROW + (((t & 7) ^ ((row >> 1) & 7)) * 8);
#pragma unroll
    for (int i = 0; i < NB; ++i) *(pair8_t*)(dst + 32 * i * IMG_WROW) = q[i];
}

// 32 k of the wave's 32 rows against the staged chunk: fragment f of step j holds row 32 f + r,
// k = 16 j + 8 h .. + 7
template <int NB>
__device__ __forceinline__ void mma_chunk(const pair_t* buf, const pair8_t (&ahi)[2], const pair8_t (&alo)[2],
                                          f32x16 (&acc)[NB], int r, int h) {
    const int swz = (r >> 1) & 7;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int f = 0; f < NB; ++f) {
            const pair_t* row = buf + (32 * f + r) * IMG_WROW;
            const pair8_t bhi = *(const pair8_t*)(row + (((2 * j + h) ^ swz) * 8));
            const pair8_t blo = *(const pair8_t*)(row + (((4 + 2 * j + h) ^ swz) * 8));
            acc[f] = mma3(ahi[j], alo[j], bhi, blo, acc[f]);
        }
}

// 32 channels from c of a pair row (xr already at the lane's 8 h): zero where the row is padding
__device__ __forceinline__ void a_load(const pair_t* xr, bool ok, int c, int lo_off, pair8_t (&hi)[2], pair8_t (&lo)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        hi[j] = zero8();
        lo[j] = zero8();
        if (ok) {
            hi[j] = *(const pair8_t*)(xr + c + 16 * j);
            lo[j] = *(const pair8_t*)(xr + lo_off + c + 16 * j);
        }
    }
}

// One workgroup: 128 output rows (4 waves x 32, row -> (b, yo, xo) decoded once; a tile may straddle a
// map-row end or an image boundary) x 32 NB columns from blockIdx.y * 32 NB: all Cout where the rows alone
// fill the device, a divisor of Cout / 32 per workgroup on small maps (cmt_img_conv3x3 picks; an output's sum
// has the same order either way).  The chunk sequence is tap-major,
// Cin / 32 chunks per tap; chunk i + 1's W pieces and A fragments are loaded while chunk i's MFMAs run,
// the pieces are written to the other LDS buffer after them.  A tap that is padding for all 32 rows of
// a wave costs that wave no A load and no MFMA (ballot); a wave past the last row still stages W and
// takes part in the barriers.
template <int NB>
__global__ __launch_bounds__(256) void img_conv3x3_kernel(cmt_img_conv_args a, int Ho, int Wo, int M) {
    __shared__ __attribute__((aligned(16))) pair_t s_w[2][NB * 32 * IMG_WROW];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int s = a.stride;
    const int n0 = blockIdx.y * (32 * NB);
    const int row0 = blockIdx.x * IMG_TM + wave * 32;
    const int m = row0 + r;
    const bool live = m < M;
    int b = 0, yo = 0, xo = 0;
    if (live) {
        b = m / (Ho * Wo);
        const int p = m - b * (Ho * Wo);
        yo = p / Wo;
        xo = p - yo * Wo;
    }
    const int Cin = a.Cin, Ktot = 9 * Cin;
    const int cpt = Cin / IMG_KC, nchunks = 9 * cpt;
    const pair_t* X = (const pair_t*)a.X;
    const pair_t* Wt = (const pair_t*)a.Wt;
    auto tap_src = [&](int tap, bool& ok) -> const pair_t* {
        const int yi = yo * s - 1 + tap / 3, xi = xo * s - 1 + tap % 3;
        ok = live && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
        return X + ((int64_t)(b * a.H + (ok ? yi : 0)) * a.W + (ok ? xi : 0)) * a.ldx + 8 * h;
    };
    f32x16 acc[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[f][i] = 0.f;

    pair8_t wq[NB], ahi[2], alo[2], nhi[2], nlo[2];
    w_load<NB>(wq, Wt, a.ldw, Ktot, n0, 0, t);
    w_store<NB>(s_w[0], wq, t);
    int tap = 0, cc = 0;
    bool ok;
    const pair_t* xr = tap_src(0, ok);
    bool any = __ballot(ok) != 0;
    a_load(xr, ok, 0, Cin, ahi, alo);
    __syncthreads();
    for (int it = 0; it < nchunks; ++it) {
        int ntap = tap, ncc = cc + 1;
        if (ncc == cpt) {
            ncc = 0;
            ++ntap;
        }
        const bool more = it + 1 < nchunks;   // workgroup-uniform
        bool nok = ok, nany = any;
        const pair_t* nxr = xr;
        if (more) {
            w_load<NB>(wq, Wt, a.ldw, Ktot, n0, ntap * Cin + IMG_KC * ncc, t);
            if (ncc == 0) {
                nxr = tap_src(ntap, nok);
                nany = __ballot(nok) != 0;
            }
            a_load(nxr, nok, IMG_KC * ncc, Cin, nhi, nlo);
        }
        if (any) mma_chunk<NB>(s_w[it & 1], ahi, alo, acc, r, h);   // wave-uniform
        // the other buffer was last read before the barrier that ended chunk it - 1
        if (more) w_store<NB>(s_w[(it + 1) & 1], wq, t);
        __syncthreads();
        tap = ntap;
        cc = ncc;
        xr = nxr;
        ok = nok;
        any = nany;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            ahi[j] = nhi[j];
            alo[j] = nlo[j];
        }
    }

    pair_t* Y = (pair_t*)a.Y;
    bool bad = false;
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        const int col = n0 + 32 * f + r;
        const float sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + acc_row(i, h);
            if (row >= M) continue;
            float v = acc[f][i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            store_pair(Y + (int64_t)row * a.ldy, a.Cout, col, v);
        }
    }
    raise_range_flag(a.range_flag, bad);
}

// One workgroup: 128 pixels of one image (grid z) x 128 output channels (grid y); the chunk sequence
// runs source by source, C_s / 32 chunks each, at k offset off_s of W.  The rest as the conv above.
// part: every wave sums its rows' stored values per column in row order, the two lane halves are
// added, the four waves' sums meet in LDS and are added in wave order: one fixed order per tile.
__global__ __launch_bounds__(256) void img_concat_kernel(cmt_img_concat_args a, int Ktot, int tiles) {
    constexpr int NB = IMG_CAT_NB;
    __shared__ __attribute__((aligned(16))) pair_t s_w[2][NB * 32 * IMG_WROW];
    __shared__ float s_part[4][32 * NB];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, n0 = blockIdx.y * (32 * NB);
    const int p0 = blockIdx.x * IMG_TM + wave * 32;
    const bool live = p0 + r < a.HW;
    const bool any = p0 < a.HW;   // wave-uniform
    const int64_t m = (int64_t)b * a.HW + (live ? p0 + r : 0);
    const pair_t* Wt = (const pair_t*)a.Wt;
    f32x16 acc[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[f][i] = 0.f;

    pair8_t wq[NB], ahi[2], alo[2], nhi[2], nlo[2];
    w_load<NB>(wq, Wt, a.ldw, Ktot, n0, 0, t);
    w_store<NB>(s_w[0], wq, t);
    int src = 0, cc = 0, off = 0, Cs = a.C[0];
    const pair_t* xr = (const pair_t*)a.X[0] + m * a.ldx[0] + 8 * h;
    a_load(xr, live, 0, Cs, ahi, alo);
    __syncthreads();
    for (int it = 0;; ++it) {
        int nsrc = src, ncc = cc + 1, noff = off, nCs = Cs;
        const pair_t* nxr = xr;
        if (IMG_KC * ncc == Cs) {
            ncc = 0;
            ++nsrc;
            noff = off + Cs;
        }
        const bool more = nsrc < a.nsrc;   // workgroup-uniform
        if (more) {
            if (ncc == 0) {
                nCs = a.C[nsrc];
                nxr = (const pair_t*)a.X[nsrc] + m * a.ldx[nsrc] + 8 * h;
            }
            w_load<NB>(wq, Wt, a.ldw, Ktot, n0, noff + IMG_KC * ncc, t);
            a_load(nxr, live, IMG_KC * ncc, nCs, nhi, nlo);
        }
        if (any) mma_chunk<NB>(s_w[it & 1], ahi, alo, acc, r, h);
        if (more) w_store<NB>(s_w[(it + 1) & 1], wq, t);
        __syncthreads();
        if (!more) break;
        src = nsrc;
        cc = ncc;
        off = noff;
        Cs = nCs;
        xr = nxr;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            ahi[j] = nhi[j];
            alo[j] = nlo[j];
        }
    }

    pair_t* Y = (pair_t*)a.Y;
    bool bad = false;
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        const int col = n0 + 32 * f + r;
        const float sh = a.shift[col];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + acc_row(i, h);
            if (p >= a.HW) continue;
            float v = acc[f][i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            pair_t hi, lo;
            split_pair(v, hi, lo);
            pair_t* row = Y + ((int64_t)b * a.HW + p) * a.ldy;
            row[col] = hi;
            row[a.Cout + col] = lo;
            sum += (float)hi + (float)lo;
        }
        sum = pair_sum(sum);
        if (h == 0) s_part[wave][32 * f + r] = sum;
    }
    raise_range_flag(a.range_flag, bad);
    if (a.part != nullptr) {   // workgroup-uniform
        __syncthreads();
        if (t < 32 * NB)
            a.part[((int64_t)b * tiles + blockIdx.x) * a.Cout + n0 + t] =
                ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
    }
}

// One workgroup: 128 output pixels (4 waves x 32) x all Cout, 32 columns at a time.  K = 9 Cin <= 27
// is padded to 32 (two MFMA steps): lane (r, h) gathers pixels k = 16 j + 8 h .. + 7 of its row's
// window, k = (ky*3 + kx) * Cin + c, splits them, and keeps both fragments for every column block.
// Lanes r run along xo, so a load's 32 addresses are every other float of one image line.
__global__ __launch_bounds__(256) void img_stem_kernel(cmt_img_stem_args a, int Ho, int Wo, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * IMG_TM + wave * 32;
    if (row0 >= M) return;   // wave-uniform; the kernel has no barrier
    const int m = row0 + r;
    const bool live = m < M;
    int b = 0, yo = 0, xo = 0;
    if (live) {
        b = m / (Ho * Wo);
        const int p = m - b * (Ho * Wo);
        yo = p / Wo;
        xo = p - yo * Wo;
    }
    const int Cin = a.Cin, K = 9 * Cin;
    const float* xb = a.X + (int64_t)b * a.x_bstride;
    bool bad = false;
    pair8_t ahi[2], alo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int k = 16 * j + 8 * h + jj;
            float v = 0.f;
            if (live && k < K) {
                const int tap = k / Cin, c = k - tap * Cin;
                const int yi = 2 * yo - 1 + tap / 3, xi = 2 * xo - 1 + tap % 3;
                if ((unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W)
                    v = xb[((int64_t)c * a.H + yi) * a.W + xi];
            }
            bad |= f16_unrepresentable(v);
            pair_t hi, lo;
            split_pair(v, hi, lo);
            ahi[j][jj] = hi;
            alo[j][jj] = lo;
        }
    pair_t* Y = (pair_t*)a.Y;
    for (int nb = 0; nb < a.Cout / 32; ++nb) {
        const int col = 32 * nb + r;
        const pair_t* wr = (const pair_t*)a.Wt + (int64_t)col * (2 * IMG_KC) + 8 * h;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc = mma3(ahi[j], alo[j], *(const pair8_t*)(wr + 16 * j), *(const pair8_t*)(wr + IMG_KC + 16 * j), acc);
        const float sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + acc_row(i, h);
            if (row >= M) continue;
            float v = acc[i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            store_pair(Y + (int64_t)row * a.ldy, a.Cout, col, v);
        }
    }
    raise_range_flag(a.range_flag, bad);
}

// One workgroup: 16 outputs of one image.  Every workgroup first sums the tiles per channel in ascending
// order (thread c, c + 256, ...: coalesced along channels) into the mean in LDS; then a wave takes four
// outputs in turn, lane l the channels l, l + 64, ... in ascending order on fp32 FMAs, and the 64 lane
// sums are folded by xor shuffles (32, 16, ... 1), a fixed order.
__global__ __launch_bounds__(256) void img_gate_kernel(cmt_img_gate_args a) {
    extern __shared__ float s_mean[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.y, C = a.C;
    const float* part = a.part + (int64_t)b * a.tiles * C;
    const float hw = (float)a.HW;
    for (int c = t; c < C; c += 256) {
        float s = 0.f;
        for (int tt = 0; tt < a.tiles; ++tt) s += part[(int64_t)tt * C + c];
        s_mean[c] = s / hw;
    }
    __syncthreads();
    for (int q = 0; q < IMG_GATE_OB / 4; ++q) {
        const int o = blockIdx.x * IMG_GATE_OB + wave * (IMG_GATE_OB / 4) + q;
        if (o >= C) break;   // wave-uniform
        const float* w = a.Wfc + (int64_t)o * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = fmaf(w[c], s_mean[c], s);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) a.gate[(int64_t)b * C + o] = fminf(fmaxf((s + a.bias[o]) + 3.f, 0.f), 6.f) / 6.f;
    }
}

// One thread: 8 channels of one pixel.  Reads come before the writes of the same elements, so Y may be X.
__global__ __launch_bounds__(256) void img_apply_kernel(cmt_img_apply_args a, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int groups = a.C / 8;
    const int64_t row = idx / groups;
    const int c = (int)(idx - row * groups) * 8;
    const int b = (int)(row / a.HW);
    const pair_t* x = (const pair_t*)a.X + row * a.ldx + c;
    const pair8_t xhi = *(const pair8_t*)x, xlo = *(const pair8_t*)(x + a.C);
    const float* g = a.gate + (int64_t)b * a.C + c;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ((float)xhi[j] + (float)xlo[j]) * g[j];
    if (a.R != nullptr) {
        const pair_t* rr = (const pair_t*)a.R + row * a.ldr + c;
        const pair8_t rhi = *(const pair8_t*)rr, rlo = *(const pair8_t*)(rr + a.C);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)rhi[j] + (float)rlo[j];
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) bad |= f16_unrepresentable(v[j]);
    store_pair8((pair_t*)a.Y + row * a.ldy, a.C, c, v);
    raise_range_flag(a.range_flag, bad);
}

// One thread: 8 channels of one output pixel.  The window starts inside the map (2 yo <= H - 2) and is
// clipped at the far edges; the maximum starts from the window's first element, never from zero.
__global__ __launch_bounds__(256) void img_pool_kernel(cmt_img_pool_args a, int Ho, int Wo, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int groups = a.C / 8;
    const int64_t m = idx / groups;
    const int c = (int)(idx - m * groups) * 8;
    const int b = (int)(m / ((int64_t)Ho * Wo));
    const int p = (int)(m - (int64_t)b * Ho * Wo);
    const int yo = p / Wo, xo = p - yo * Wo;
    const pair_t* X = (const pair_t*)a.X;
    pair8_t bhi, blo;
    float bv[8];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int yi = 2 * yo + dy, xi = 2 * xo + dx;
            if (yi >= a.H || xi >= a.W) continue;
            const pair_t* x = X + ((int64_t)(b * a.H + yi) * a.W + xi) * a.ldx + c;
            const pair8_t hi = *(const pair8_t*)x, lo = *(const pair8_t*)(x + a.C);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)hi[j] + (float)lo[j];
                if ((dy == 0 && dx == 0) || v > bv[j] || v != v) {
                    bv[j] = v;
                    bhi[j] = hi[j];
                    blo[j] = lo[j];
                }
            }
        }
    pair_t* y = (pair_t*)a.Y + m * a.ldy + c;
    *(pair8_t*)y = bhi;
    *(pair8_t*)(y + a.C) = blo;
}

template <typename T>
bool img_aligned16(const T* p) { return (((uintptr_t)p) & 15) == 0; }

template <int NB>
void img_conv_launch(const cmt_img_conv_args* a, int Ho, int Wo, int64_t M, hipStream_t s) {
    img_conv3x3_kernel<NB><<<dim3((unsigned)cdiv64(M, IMG_TM), (unsigned)(a->Cout / (32 * NB))), 256, 0, s>>>(*a, Ho, Wo, (int)M);
}

}  // namespace

extern "C" int64_t cmt_img_stem_args_size(void) { return (int64_t)sizeof(cmt_img_stem_args); }
extern "C" int64_t cmt_img_conv_args_size(void) { return (int64_t)sizeof(cmt_img_conv_args); }
extern "C" int64_t cmt_img_concat_args_size(void) { return (int64_t)sizeof(cmt_img_concat_args); }
extern "C" int64_t cmt_img_gate_args_size(void) { return (int64_t)sizeof(cmt_img_gate_args); }
extern "C" int64_t cmt_img_apply_args_size(void) { return (int64_t)sizeof(cmt_img_apply_args); }
extern "C" int64_t cmt_img_pool_args_size(void) { return (int64_t)sizeof(cmt_img_pool_args); }
extern "C" int cmt_img_concat_tile_rows(void) { return IMG_TM; }

extern "C" int cmt_img_stem(const cmt_img_stem_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_stem: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->Y, "cmt_img_stem: X, Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_img_stem: B, H and W must be positive");
    CMT_REQUIRE(a->Cin >= 1 && a->Cin <= 3, "cmt_img_stem: Cin must be 1, 2 or 3");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % 32 == 0, "cmt_img_stem: Cout must be a positive multiple of 32");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_img_stem: B*H*W must be below 2^31");
    CMT_REQUIRE(a->x_bstride >= (int64_t)a->Cin * a->H * a->W, "cmt_img_stem: x_bstride below Cin*H*W");
    CMT_REQUIRE(a->ldy >= 2 * (int64_t)a->Cout, "cmt_img_stem: ldy >= 2 Cout required");
    CMT_REQUIRE(img_aligned16(a->Wt) && (((uintptr_t)a->X) & 3) == 0 && (((uintptr_t)a->Y) & 1) == 0,
                "cmt_img_stem: Wt must be 16-byte, X 4-byte and Y 2-byte aligned");
    const int Ho = (a->H - 1) / 2 + 1, Wo = (a->W - 1) / 2 + 1;
    const int64_t M = (int64_t)a->B * Ho * Wo;
    img_stem_kernel<<<dim3((unsigned)cdiv64(M, IMG_TM)), 256, 0, (hipStream_t)stream>>>(*a, Ho, Wo, (int)M);
    return cmt_check_launch("cmt_img_stem");
}

extern "C" int cmt_img_conv3x3(const cmt_img_conv_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_conv3x3: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->Y, "cmt_img_conv3x3: X, Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_img_conv3x3: B, H and W must be positive");
    CMT_REQUIRE(a->stride == 1 || a->stride == 2, "cmt_img_conv3x3: stride must be 1 or 2");
    CMT_REQUIRE(a->Cin > 0 && a->Cin % 32 == 0, "cmt_img_conv3x3: Cin must be a positive multiple of 32");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % 32 == 0 && a->Cout <= 256,
                "cmt_img_conv3x3: Cout must be a positive multiple of 32, at most 256");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_img_conv3x3: B*H*W must be below 2^31");
    CMT_REQUIRE(a->ldx >= 2 * (int64_t)a->Cin && a->ldx % 8 == 0 && a->ldw >= 18 * (int64_t)a->Cin && a->ldw % 8 == 0 &&
                    a->ldy >= 2 * (int64_t)a->Cout,
                "cmt_img_conv3x3: ldx >= 2 Cin, ldw >= 18 Cin (both % 8, 16-bit words) and ldy >= 2 Cout required");
    CMT_REQUIRE(img_aligned16(a->X) && img_aligned16(a->Wt) && (((uintptr_t)a->Y) & 1) == 0,
                "cmt_img_conv3x3: X and Wt must be 16-byte aligned");
    const int s = a->stride;
    const int Ho = (a->H - 1) / s + 1, Wo = (a->W - 1) / s + 1;
    const int64_t M = (int64_t)a->B * Ho * Wo;
    hipStream_t st = (hipStream_t)stream;
    // column blocks per workgroup: all of them, unless the row tiles alone leave compute units idle; then the
    // largest divisor of Cout / 32 that gives every unit a workgroup (or 1).  Measured at the V-99-eSE shapes
    // (DESIGN 12): 188 tiles of 192 columns run 1.24 x faster as 3 + 3, 47 tiles of 224 1.8 x faster as 7 x 1.
    const int blocks = a->Cout / 32;
    int nb = a->nb;
    CMT_REQUIRE(nb >= 0 && (nb == 0 || blocks % nb == 0), "cmt_img_conv3x3: nb must be 0 or a divisor of Cout / 32");
    if (nb == 0) {
        const int64_t tiles = cdiv64(M, IMG_TM), cus = cmt_cu_count();
        nb = blocks;
        if (tiles < cus) {
            nb = 1;
            for (int d = blocks; d > 1; --d)
                if (blocks % d == 0 && tiles * (blocks / d) >= cus) {
                    nb = d;
                    break;
                }
        }
    }
    switch (nb) {
        case 1: img_conv_launch<1>(a, Ho, Wo, M, st); break;
        case 2: img_conv_launch<2>(a, Ho, Wo, M, st); break;
        case 3: img_conv_launch<3>(a, Ho, Wo, M, st); break;
        case 4: img_conv_launch<4>(a, Ho, Wo, M, st); break;
        case 5: img_conv_launch<5>(a, Ho, Wo, M, st); break;
        case 6: img_conv_launch<6>(a, Ho, Wo, M, st); break;
        case 7: img_conv_launch<7>(a, Ho, Wo, M, st); break;
        default: img_conv_launch<8>(a, Ho, Wo, M, st); break;
    }
    return cmt_check_launch("cmt_img_conv3x3");
}

extern "C" int cmt_img_concat1x1(const cmt_img_concat_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_concat1x1: null argument struct");
    CMT_REQUIRE(a->Wt && a->shift && a->Y, "cmt_img_concat1x1: Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->HW > 0, "cmt_img_concat1x1: B and HW must be positive");
    CMT_REQUIRE(a->B <= 65535, "cmt_img_concat1x1: B beyond the grid");
    CMT_REQUIRE(a->nsrc >= 1 && a->nsrc <= CMT_IMG_MAX_SRC, "cmt_img_concat1x1: 1 to 8 sources required");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % (32 * IMG_CAT_NB) == 0, "cmt_img_concat1x1: Cout must be a positive multiple of 128");
    CMT_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), "cmt_img_concat1x1: B*HW must be below 2^31");
    int64_t K = 0;
    for (int s = 0; s < a->nsrc; ++s) {
        CMT_REQUIRE(a->X[s] != nullptr && img_aligned16(a->X[s]), "cmt_img_concat1x1: every source must be non-null and 16-byte aligned");
        CMT_REQUIRE(a->C[s] > 0 && a->C[s] % 32 == 0, "cmt_img_concat1x1: every source width must be a positive multiple of 32");
        CMT_REQUIRE(a->ldx[s] >= 2 * (int64_t)a->C[s] && a->ldx[s] % 8 == 0, "cmt_img_concat1x1: ldx >= 2 C and % 8 (16-bit words) required");
        K += a->C[s];
    }
    CMT_REQUIRE(K < ((int64_t)1 << 24), "cmt_img_concat1x1: K too large");
    CMT_REQUIRE(a->ldw >= 2 * K && a->ldw % 8 == 0 && a->ldy >= 2 * (int64_t)a->Cout,
                "cmt_img_concat1x1: ldw >= 2 K (% 8, 16-bit words) and ldy >= 2 Cout required");
    CMT_REQUIRE(img_aligned16(a->Wt) && (((uintptr_t)a->Y) & 1) == 0 && (((uintptr_t)a->part) & 3) == 0,
                "cmt_img_concat1x1: Wt must be 16-byte aligned, part 4-byte");
    const int tiles = cdiv(a->HW, IMG_TM);
    dim3 grid((unsigned)tiles, (unsigned)(a->Cout / (32 * IMG_CAT_NB)), (unsigned)a->B);
    img_concat_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(*a, (int)K, tiles);
    return cmt_check_launch("cmt_img_concat1x1");
}

extern "C" int cmt_img_ese_gate(const cmt_img_gate_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_ese_gate: null argument struct");
    CMT_REQUIRE(a->part && a->Wfc && a->bias && a->gate, "cmt_img_ese_gate: part, Wfc, bias and gate must be non-null");
    CMT_REQUIRE(a->B > 0 && a->B <= 65535 && a->tiles > 0 && a->HW > 0, "cmt_img_ese_gate: B (<= 65535), tiles and HW must be positive");
    CMT_REQUIRE(a->C > 0 && a->C % 4 == 0 && a->C <= 8192, "cmt_img_ese_gate: C must be a positive multiple of 4, at most 8192");
    dim3 grid((unsigned)cdiv(a->C, IMG_GATE_OB), (unsigned)a->B);
    img_gate_kernel<<<grid, 256, (size_t)a->C * sizeof(float), (hipStream_t)stream>>>(*a);
    return cmt_check_launch("cmt_img_ese_gate");
}

extern "C" int cmt_img_ese_apply(const cmt_img_apply_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_ese_apply: null argument struct");
    CMT_REQUIRE(a->X && a->gate && a->Y, "cmt_img_ese_apply: X, gate and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->HW > 0, "cmt_img_ese_apply: B and HW must be positive");
    CMT_REQUIRE(a->C > 0 && a->C % 8 == 0, "cmt_img_ese_apply: C must be a positive multiple of 8");
    CMT_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), "cmt_img_ese_apply: B*HW must be below 2^31");
    CMT_REQUIRE(a->ldx >= 2 * (int64_t)a->C && a->ldx % 8 == 0 && a->ldy >= 2 * (int64_t)a->C && a->ldy % 8 == 0,
                "cmt_img_ese_apply: ldx, ldy >= 2 C and % 8 (16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->X) && img_aligned16(a->Y) && img_aligned16(a->gate),
                "cmt_img_ese_apply: X, Y and gate must be 16-byte aligned");
    if (a->R != nullptr)
        CMT_REQUIRE(a->ldr >= 2 * (int64_t)a->C && a->ldr % 8 == 0 && img_aligned16(a->R),
                    "cmt_img_ese_apply: ldr >= 2 C, % 8, and a 16-byte aligned R required");
    const int64_t total = (int64_t)a->B * a->HW * (a->C / 8);
    const int64_t blocks = cdiv64(total, 256);
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), "cmt_img_ese_apply: grid too large");
    img_apply_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, total);
    return cmt_check_launch("cmt_img_ese_apply");
}

extern "C" int cmt_img_maxpool(const cmt_img_pool_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_maxpool: null argument struct");
    CMT_REQUIRE(a->X && a->Y, "cmt_img_maxpool: X and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H >= 2 && a->W >= 2, "cmt_img_maxpool: B positive and H, W >= 2 required");
    CMT_REQUIRE(a->C > 0 && a->C % 8 == 0, "cmt_img_maxpool: C must be a positive multiple of 8");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_img_maxpool: B*H*W must be below 2^31");
    CMT_REQUIRE(a->ldx >= 2 * (int64_t)a->C && a->ldx % 8 == 0 && a->ldy >= 2 * (int64_t)a->C && a->ldy % 8 == 0,
                "cmt_img_maxpool: ldx, ldy >= 2 C and % 8 (16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->X) && img_aligned16(a->Y), "cmt_img_maxpool: X and Y must be 16-byte aligned");
    const int Ho = (a->H - 2) / 2 + 1, Wo = (a->W - 2) / 2 + 1;
    const int64_t total = (int64_t)a->B * Ho * Wo * (a->C / 8);
    const int64_t blocks = cdiv64(total, 256);
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), "cmt_img_maxpool: grid too large");
    img_pool_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, Ho, Wo, total);
    return cmt_check_launch("cmt_img_maxpool");
}

// ---- the one-pass fp16 policy (cmt_img_*_f16) -------------------------------------------------------------------
// The same launches on plain fp16 rows [B*H*W][C] with W rounded once to fp16: one MFMA per 16-k step instead
// of three, 2 bytes per activation between layers instead of 4.  The tile (128 rows per workgroup, 32 per wave,
// NB accumulators of 32 columns), the LDS row of 128 bytes with its XOR swizzle (w_store above, unchanged) and
// the double buffer are those of the three-pass kernels; a staged chunk holds 64 k instead of hi | lo of 32, so
// a chunk carries four MFMA steps per accumulator and the barrier, staging and gather cost per MFMA stays at
// 3/4 of the three-pass kernel's instead of tripling.  A channel count with C % 64 == 32 ends in a half chunk
// (32 k: pieces 4 .. 7 of the LDS row are neither loaded nor read).  K order: tap-major (source-major), channels
// ascending, as above.
namespace {

constexpr int IMG_KC16 = 64;    // k per staged chunk of fp16 W (four 16-k steps)

// A W chunk of plain fp16 rows: rows [n0, n0 + 32 NB) x 64 k from k offset kb of [N][ldw].  Piece i of thread
// t: row (t >> 3) + 32 i, 16 bytes sub = t & 7 of the row's 128; a half chunk has pieces 0 .. 3 only (the
// others would lie in the next tap or past the row's end) and leaves the registers as they are.
template <int NB>
__device__ __forceinline__ void w_load16(pair8_t (&q)[NB], const f16_t* Wt, int64_t ldw, int n0, int kb, bool half, int t) {
    const int sub = t & 7;
    if (half && sub >= 4) return;
    const f16_t* src = Wt + (int64_t)(n0 + (t >> 3)) * ldw + kb + 8 * sub;
#pragma unroll
    for (int i = 0; i < NB; ++i) q[i] = *(const pair8_t*)(src + (int64_t)(32 * i) * ldw);
}

// 64 k (a half chunk: 32) of the wave's 32 rows against the staged chunk: step j is k = 16 j + 8 h .. + 7,
// piece 2 j + h of the row
template <int NB>
__device__ __forceinline__ void mma_chunk16(const f16_t* buf, const pair8_t (&a)[4], f32x16 (&acc)[NB], bool half, int r, int h) {
    const int swz = (r >> 1) & 7;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= 2 && half) break;   // workgroup-uniform
#pragma unroll
        for (int f = 0; f < NB; ++f) {
            const pair8_t b = *(const pair8_t*)(buf + (32 * f + r) * IMG_WROW + (((2 * j + h) ^ swz) * 8));
            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[j], b, acc[f], 0, 0, 0);
        }
    }
}

// 64 (a half chunk: 32) channels from c of an fp16 row (xr already at the lane's 8 h): zero where the row is padding
__device__ __forceinline__ void a_load16(const f16_t* xr, bool ok, int c, bool half, pair8_t (&a)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = zero8();
        if (ok && !(half && j >= 2)) a[j] = *(const pair8_t*)(xr + c + 16 * j);
    }
}

// img_conv3x3_kernel on fp16 rows: ceil(Cin / 64) chunks per tap, the last a half chunk where Cin % 64 == 32.
template <int NB>
__global__ __launch_bounds__(256, NB >= 5 ? 2 : (NB >= 3 ? 3 : 4)) void img_conv3x3_f16_kernel(cmt_img_conv_args a, int Ho, int Wo, int M) {
    __shared__ __attribute__((aligned(16))) f16_t s_w[2][NB * 32 * IMG_WROW];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int s = a.stride;
    const int n0 = blockIdx.y * (32 * NB);
    const int row0 = blockIdx.x * IMG_TM + wave * 32;
    const int m = row0 + r;
    const bool live = m < M;
    int b = 0, yo = 0, xo = 0;
    if (live) {
        b = m / (Ho * Wo);
        const int p = m - b * (Ho * Wo);
        yo = p / Wo;
        xo = p - yo * Wo;
    }
    const int Cin = a.Cin;
    const int cpt = (Cin + IMG_KC16 - 1) / IMG_KC16, nchunks = 9 * cpt;
    const bool odd = (Cin % IMG_KC16) != 0;   // the last chunk of every tap is a half chunk
    const f16_t* X = (const f16_t*)a.X;
    const f16_t* Wt = (const f16_t*)a.Wt;
    auto tap_src = [&](int tap, bool& ok) -> const f16_t* {
        const int yi = yo * s - 1 + tap / 3, xi = xo * s - 1 + tap % 3;
        ok = live && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
        return X + ((int64_t)(b * a.H + (ok ? yi : 0)) * a.W + (ok ? xi : 0)) * a.ldx + 8 * h;
    };
    f32x16 acc[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[f][i] = 0.f;

    pair8_t wq[NB], av[4], nv[4];
#pragma unroll
    for (int i = 0; i < NB; ++i) wq[i] = zero8();
    bool half = odd && cpt == 1;
    w_load16<NB>(wq, Wt, a.ldw, n0, 0, half, t);
    w_store<NB>(s_w[0], wq, t);
    int tap = 0, cc = 0;
    bool ok;
    const f16_t* xr = tap_src(0, ok);
    bool any = __ballot(ok) != 0;
    a_load16(xr, ok, 0, half, av);
    __syncthreads();
    for (int it = 0; it < nchunks; ++it) {
        int ntap = tap, ncc = cc + 1;
        if (ncc == cpt) {
            ncc = 0;
            ++ntap;
        }
        const bool more = it + 1 < nchunks;   // workgroup-uniform
        const bool nhalf = odd && ncc == cpt - 1;
        bool nok = ok, nany = any;
        const f16_t* nxr = xr;
        if (more) {
            w_load16<NB>(wq, Wt, a.ldw, n0, ntap * Cin + IMG_KC16 * ncc, nhalf, t);
            if (ncc == 0) {
                nxr = tap_src(ntap, nok);
                nany = __ballot(nok) != 0;
            }
            a_load16(nxr, nok, IMG_KC16 * ncc, nhalf, nv);
        }
        if (any) mma_chunk16<NB>(s_w[it & 1], av, acc, half, r, h);   // wave-uniform
        // the other buffer was last read before the barrier that ended chunk it - 1
        if (more) w_store<NB>(s_w[(it + 1) & 1], wq, t);
        __syncthreads();
        tap = ntap;
        cc = ncc;
        xr = nxr;
        ok = nok;
        any = nany;
        half = nhalf;
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = nv[j];
    }

    f16_t* Y = (f16_t*)a.Y;
    bool bad = false;
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        const int col = n0 + 32 * f + r;
        const float sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + acc_row(i, h);
            if (row >= M) continue;
            float v = acc[f][i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            Y[(int64_t)row * a.ldy + col] = (f16_t)v;
        }
    }
    raise_range_flag(a.range_flag, bad);
}

// img_concat_kernel on fp16 rows: ceil(C_s / 64) chunks per source, the last a half chunk where C_s % 64 == 32.
// part: the fp32 sums of the fp16 values as stored, in the order of the three-pass kernel.
__global__ __launch_bounds__(256) void img_concat_f16_kernel(cmt_img_concat_args a, int tiles) {
    constexpr int NB = IMG_CAT_NB;
    __shared__ __attribute__((aligned(16))) f16_t s_w[2][NB * 32 * IMG_WROW];
    __shared__ float s_part[4][32 * NB];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, n0 = blockIdx.y * (32 * NB);
    const int p0 = blockIdx.x * IMG_TM + wave * 32;
    const bool live = p0 + r < a.HW;
    const bool any = p0 < a.HW;   // wave-uniform
    const int64_t m = (int64_t)b * a.HW + (live ? p0 + r : 0);
    const f16_t* Wt = (const f16_t*)a.Wt;
    f32x16 acc[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[f][i] = 0.f;

    pair8_t wq[NB], av[4], nv[4];
#pragma unroll
    for (int i = 0; i < NB; ++i) wq[i] = zero8();
    int src = 0, cc = 0, off = 0, Cs = a.C[0];
    bool half = Cs - IMG_KC16 * cc < IMG_KC16;
    w_load16<NB>(wq, Wt, a.ldw, n0, 0, half, t);
    w_store<NB>(s_w[0], wq, t);
    const f16_t* xr = (const f16_t*)a.X[0] + m * a.ldx[0] + 8 * h;
    a_load16(xr, live, 0, half, av);
    __syncthreads();
    for (int it = 0;; ++it) {
        int nsrc = src, ncc = cc + 1, noff = off, nCs = Cs;
        const f16_t* nxr = xr;
        if (IMG_KC16 * ncc >= Cs) {
            ncc = 0;
            ++nsrc;
            noff = off + Cs;
        }
        const bool more = nsrc < a.nsrc;   // workgroup-uniform
        bool nhalf = false;
        if (more) {
            if (ncc == 0) {
                nCs = a.C[nsrc];
                nxr = (const f16_t*)a.X[nsrc] + m * a.ldx[nsrc] + 8 * h;
            }
            nhalf = nCs - IMG_KC16 * ncc < IMG_KC16;
            w_load16<NB>(wq, Wt, a.ldw, n0, noff + IMG_KC16 * ncc, nhalf, t);
            a_load16(nxr, live, IMG_KC16 * ncc, nhalf, nv);
        }
        if (any) mma_chunk16<NB>(s_w[it & 1], av, acc, half, r, h);
        if (more) w_store<NB>(s_w[(it + 1) & 1], wq, t);
        __syncthreads();
        if (!more) break;
        src = nsrc;
        cc = ncc;
        off = noff;
        Cs = nCs;
        xr = nxr;
        half = nhalf;
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = nv[j];
    }

    f16_t* Y = (f16_t*)a.Y;
    bool bad = false;
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        const int col = n0 + 32 * f + r;
        const float sh = a.shift[col];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + acc_row(i, h);
            if (p >= a.HW) continue;
            float v = acc[f][i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            const f16_t y = (f16_t)v;
            Y[((int64_t)b * a.HW + p) * a.ldy + col] = y;
            sum += (float)y;
        }
        sum = pair_sum(sum);
        if (h == 0) s_part[wave][32 * f + r] = sum;
    }
    raise_range_flag(a.range_flag, bad);
    if (a.part != nullptr) {   // workgroup-uniform
        __syncthreads();
        if (t < 32 * NB)
            a.part[((int64_t)b * tiles + blockIdx.x) * a.Cout + n0 + t] =
                ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
    }
}

// img_stem_kernel with every pixel rounded once to fp16 and W fp16 [Cout][32]: one MFMA per step
__global__ __launch_bounds__(256) void img_stem_f16_kernel(cmt_img_stem_args a, int Ho, int Wo, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * IMG_TM + wave * 32;
    if (row0 >= M) return;   // wave-uniform; the kernel has no barrier
    const int m = row0 + r;
    const bool live = m < M;
    int b = 0, yo = 0, xo = 0;
    if (live) {
        b = m / (Ho * Wo);
        const int p = m - b * (Ho * Wo);
        yo = p / Wo;
        xo = p - yo * Wo;
    }
    const int Cin = a.Cin, K = 9 * Cin;
    const float* xb = a.X + (int64_t)b * a.x_bstride;
    bool bad = false;
    pair8_t av[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int k = 16 * j + 8 * h + jj;
            float v = 0.f;
            if (live && k < K) {
                const int tap = k / Cin, c = k - tap * Cin;
                const int yi = 2 * yo - 1 + tap / 3, xi = 2 * xo - 1 + tap % 3;
                if ((unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W)
                    v = xb[((int64_t)c * a.H + yi) * a.W + xi];
            }
            bad |= f16_unrepresentable(v);
            av[j][jj] = (f16_t)v;
        }
    f16_t* Y = (f16_t*)a.Y;
    for (int nb = 0; nb < a.Cout / 32; ++nb) {
        const int col = 32 * nb + r;
        const f16_t* wr = (const f16_t*)a.Wt + (int64_t)col * IMG_KC + 8 * h;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[j], *(const pair8_t*)(wr + 16 * j), acc, 0, 0, 0);
        const float sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + acc_row(i, h);
            if (row >= M) continue;
            float v = acc[i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            Y[(int64_t)row * a.ldy + col] = (f16_t)v;
        }
    }
    raise_range_flag(a.range_flag, bad);
}

// One thread: 8 channels of one pixel, fp32 multiply and add, one rounding.  Reads come before the writes of
// the same elements, so Y may be X.
__global__ __launch_bounds__(256) void img_apply_f16_kernel(cmt_img_apply_args a, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int groups = a.C / 8;
    const int64_t row = idx / groups;
    const int c = (int)(idx - row * groups) * 8;
    const int b = (int)(row / a.HW);
    const pair8_t x = *(const pair8_t*)((const f16_t*)a.X + row * a.ldx + c);
    const float* g = a.gate + (int64_t)b * a.C + c;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)x[j] * g[j];
    if (a.R != nullptr) {
        const pair8_t rr = *(const pair8_t*)((const f16_t*)a.R + row * a.ldr + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)rr[j];
    }
    bool bad = false;
    pair8_t y;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bad |= f16_unrepresentable(v[j]);
        y[j] = (f16_t)v[j];
    }
    *(pair8_t*)((f16_t*)a.Y + row * a.ldy + c) = y;
    raise_range_flag(a.range_flag, bad);
}

// One thread: 8 channels of one output pixel; img_pool_kernel's window on fp16 values, copied unchanged.
__global__ __launch_bounds__(256) void img_pool_f16_kernel(cmt_img_pool_args a, int Ho, int Wo, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int groups = a.C / 8;
    const int64_t m = idx / groups;
    const int c = (int)(idx - m * groups) * 8;
    const int b = (int)(m / ((int64_t)Ho * Wo));
    const int p = (int)(m - (int64_t)b * Ho * Wo);
    const int yo = p / Wo, xo = p - yo * Wo;
    const f16_t* X = (const f16_t*)a.X;
    pair8_t best = *(const pair8_t*)(X + ((int64_t)(b * a.H + 2 * yo) * a.W + 2 * xo) * a.ldx + c);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int yi = 2 * yo + dy, xi = 2 * xo + dx;
            if ((dy == 0 && dx == 0) || yi >= a.H || xi >= a.W) continue;
            const pair8_t x = *(const pair8_t*)(X + ((int64_t)(b * a.H + yi) * a.W + xi) * a.ldx + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)x[j];
                if (v > (float)best[j] || v != v) best[j] = x[j];
            }
        }
    *(pair8_t*)((f16_t*)a.Y + m * a.ldy + c) = best;
}

template <int NB>
void img_conv_f16_launch(const cmt_img_conv_args* a, int Ho, int Wo, int64_t M, hipStream_t s) {
    img_conv3x3_f16_kernel<NB><<<dim3((unsigned)cdiv64(M, IMG_TM), (unsigned)(a->Cout / (32 * NB))), 256, 0, s>>>(*a, Ho, Wo, (int)M);
}

}  // namespace

extern "C" int cmt_img_stem_f16(const cmt_img_stem_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_stem_f16: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->Y, "cmt_img_stem_f16: X, Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_img_stem_f16: B, H and W must be positive");
    CMT_REQUIRE(a->Cin >= 1 && a->Cin <= 3, "cmt_img_stem_f16: Cin must be 1, 2 or 3");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % 32 == 0, "cmt_img_stem_f16: Cout must be a positive multiple of 32");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_img_stem_f16: B*H*W must be below 2^31");
    CMT_REQUIRE(a->x_bstride >= (int64_t)a->Cin * a->H * a->W, "cmt_img_stem_f16: x_bstride below Cin*H*W");
    CMT_REQUIRE(a->ldy >= (int64_t)a->Cout && a->ldy % 8 == 0, "cmt_img_stem_f16: ldy >= Cout and % 8 (16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->Wt) && (((uintptr_t)a->X) & 3) == 0 && (((uintptr_t)a->Y) & 1) == 0,
                "cmt_img_stem_f16: Wt must be 16-byte, X 4-byte and Y 2-byte aligned");
    const int Ho = (a->H - 1) / 2 + 1, Wo = (a->W - 1) / 2 + 1;
    const int64_t M = (int64_t)a->B * Ho * Wo;
    img_stem_f16_kernel<<<dim3((unsigned)cdiv64(M, IMG_TM)), 256, 0, (hipStream_t)stream>>>(*a, Ho, Wo, (int)M);
    return cmt_check_launch("cmt_img_stem_f16");
}

extern "C" int cmt_img_conv3x3_f16(const cmt_img_conv_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_conv3x3_f16: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->Y, "cmt_img_conv3x3_f16: X, Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_img_conv3x3_f16: B, H and W must be positive");
    CMT_REQUIRE(a->stride == 1 || a->stride == 2, "cmt_img_conv3x3_f16: stride must be 1 or 2");
    CMT_REQUIRE(a->Cin > 0 && a->Cin % 32 == 0, "cmt_img_conv3x3_f16: Cin must be a positive multiple of 32");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % 32 == 0 && a->Cout <= 256,
                "cmt_img_conv3x3_f16: Cout must be a positive multiple of 32, at most 256");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_img_conv3x3_f16: B*H*W must be below 2^31");
    CMT_REQUIRE(a->ldx >= (int64_t)a->Cin && a->ldx % 8 == 0 && a->ldw >= 9 * (int64_t)a->Cin && a->ldw % 8 == 0 &&
                    a->ldy >= (int64_t)a->Cout && a->ldy % 8 == 0,
                "cmt_img_conv3x3_f16: ldx >= Cin, ldw >= 9 Cin and ldy >= Cout (all % 8, 16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->X) && img_aligned16(a->Wt) && (((uintptr_t)a->Y) & 1) == 0,
                "cmt_img_conv3x3_f16: X and Wt must be 16-byte aligned");
    const int s = a->stride;
    const int Ho = (a->H - 1) / s + 1, Wo = (a->W - 1) / s + 1;
    const int64_t M = (int64_t)a->B * Ho * Wo;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = a->Cout / 32;
    int nb = a->nb;
    CMT_REQUIRE(nb >= 0 && (nb == 0 || blocks % nb == 0), "cmt_img_conv3x3_f16: nb must be 0 or a divisor of Cout / 32");
    if (nb == 0) {
        // as cmt_img_conv3x3: all columns per workgroup unless the row tiles alone leave compute units idle
        const int64_t tiles = cdiv64(M, IMG_TM), cus = cmt_cu_count();
        nb = blocks;
        if (tiles < cus) {
            nb = 1;
            for (int d = blocks; d > 1; --d)
                if (blocks % d == 0 && tiles * (blocks / d) >= cus) {
                    nb = d;
                    break;
                }
        }
    }
    switch (nb) {
        case 1: img_conv_f16_launch<1>(a, Ho, Wo, M, st); break;
        case 2: img_conv_f16_launch<2>(a, Ho, Wo, M, st); break;
        case 3: img_conv_f16_launch<3>(a, Ho, Wo, M, st); break;
        case 4: img_conv_f16_launch<4>(a, Ho, Wo, M, st); break;
        case 5: img_conv_f16_launch<5>(a, Ho, Wo, M, st); break;
        case 6: img_conv_f16_launch<6>(a, Ho, Wo, M, st); break;
        case 7: img_conv_f16_launch<7>(a, Ho, Wo, M, st); break;
        default: img_conv_f16_launch<8>(a, Ho, Wo, M, st); break;
    }
    return cmt_check_launch("cmt_img_conv3x3_f16");
}

extern "C" int cmt_img_concat1x1_f16(const cmt_img_concat_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_concat1x1_f16: null argument struct");
    CMT_REQUIRE(a->Wt && a->shift && a->Y, "cmt_img_concat1x1_f16: Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->HW > 0, "cmt_img_concat1x1_f16: B and HW must be positive");
    CMT_REQUIRE(a->B <= 65535, "cmt_img_concat1x1_f16: B beyond the grid");
    CMT_REQUIRE(a->nsrc >= 1 && a->nsrc <= CMT_IMG_MAX_SRC, "cmt_img_concat1x1_f16: 1 to 8 sources required");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % (32 * IMG_CAT_NB) == 0, "cmt_img_concat1x1_f16: Cout must be a positive multiple of 128");
    CMT_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), "cmt_img_concat1x1_f16: B*HW must be below 2^31");
    int64_t K = 0;
    for (int s = 0; s < a->nsrc; ++s) {
        CMT_REQUIRE(a->X[s] != nullptr && img_aligned16(a->X[s]), "cmt_img_concat1x1_f16: every source must be non-null and 16-byte aligned");
        CMT_REQUIRE(a->C[s] > 0 && a->C[s] % 32 == 0, "cmt_img_concat1x1_f16: every source width must be a positive multiple of 32");
        CMT_REQUIRE(a->ldx[s] >= (int64_t)a->C[s] && a->ldx[s] % 8 == 0, "cmt_img_concat1x1_f16: ldx >= C and % 8 (16-bit words) required");
        K += a->C[s];
    }
    CMT_REQUIRE(K < ((int64_t)1 << 24), "cmt_img_concat1x1_f16: K too large");
    CMT_REQUIRE(a->ldw >= K && a->ldw % 8 == 0 && a->ldy >= (int64_t)a->Cout && a->ldy % 8 == 0,
                "cmt_img_concat1x1_f16: ldw >= K and ldy >= Cout (both % 8, 16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->Wt) && (((uintptr_t)a->Y) & 1) == 0 && (((uintptr_t)a->part) & 3) == 0,
                "cmt_img_concat1x1_f16: Wt must be 16-byte aligned, part 4-byte");
    const int tiles = cdiv(a->HW, IMG_TM);
    dim3 grid((unsigned)tiles, (unsigned)(a->Cout / (32 * IMG_CAT_NB)), (unsigned)a->B);
    img_concat_f16_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(*a, tiles);
    return cmt_check_launch("cmt_img_concat1x1_f16");
}

extern "C" int cmt_img_ese_apply_f16(const cmt_img_apply_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_ese_apply_f16: null argument struct");
    CMT_REQUIRE(a->X && a->gate && a->Y, "cmt_img_ese_apply_f16: X, gate and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->HW > 0, "cmt_img_ese_apply_f16: B and HW must be positive");
    CMT_REQUIRE(a->C > 0 && a->C % 8 == 0, "cmt_img_ese_apply_f16: C must be a positive multiple of 8");
    CMT_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), "cmt_img_ese_apply_f16: B*HW must be below 2^31");
    CMT_REQUIRE(a->ldx >= (int64_t)a->C && a->ldx % 8 == 0 && a->ldy >= (int64_t)a->C && a->ldy % 8 == 0,
                "cmt_img_ese_apply_f16: ldx, ldy >= C and % 8 (16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->X) && img_aligned16(a->Y) && img_aligned16(a->gate),
                "cmt_img_ese_apply_f16: X, Y and gate must be 16-byte aligned");
    if (a->R != nullptr)
        CMT_REQUIRE(a->ldr >= (int64_t)a->C && a->ldr % 8 == 0 && img_aligned16(a->R),
                    "cmt_img_ese_apply_f16: ldr >= C, % 8, and a 16-byte aligned R required");
    const int64_t total = (int64_t)a->B * a->HW * (a->C / 8);
    const int64_t blocks = cdiv64(total, 256);
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), "cmt_img_ese_apply_f16: grid too large");
    img_apply_f16_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, total);
    return cmt_check_launch("cmt_img_ese_apply_f16");
}

extern "C" int cmt_img_maxpool_f16(const cmt_img_pool_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_maxpool_f16: null argument struct");
    CMT_REQUIRE(a->X && a->Y, "cmt_img_maxpool_f16: X and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H >= 2 && a->W >= 2, "cmt_img_maxpool_f16: B positive and H, W >= 2 required");
    CMT_REQUIRE(a->C > 0 && a->C % 8 == 0, "cmt_img_maxpool_f16: C must be a positive multiple of 8");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_img_maxpool_f16: B*H*W must be below 2^31");
    CMT_REQUIRE(a->ldx >= (int64_t)a->C && a->ldx % 8 == 0 && a->ldy >= (int64_t)a->C && a->ldy % 8 == 0,
                "cmt_img_maxpool_f16: ldx, ldy >= C and % 8 (16-bit words) required");
    CMT_REQUIRE(img_aligned16(a->X) && img_aligned16(a->Y), "cmt_img_maxpool_f16: X and Y must be 16-byte aligned");
    const int Ho = (a->H - 2) / 2 + 1, Wo = (a->W - 2) / 2 + 1;
    const int64_t total = (int64_t)a->B * Ho * Wo * (a->C / 8);
    const int64_t blocks = cdiv64(total, 256);
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), "cmt_img_maxpool_f16: grid too large");
    img_pool_f16_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, Ho, Wo, total);
    return cmt_check_launch("cmt_img_maxpool_f16");
}
