// Dense BEV backbone / neck kernels (mmdet3d SECOND and SECONDFPN between the SparseEncoder's
// map and the head's shared_conv), declared in include/cmt_hip.h (cmt_bev_*):
//   bev_conv3x3_kernel   3 x 3 / pad 1 conv of stride 1 or 2 from CMT_F16P NHWC rows to pair rows
//   bev_deblock_kernel   k x k / stride k transposed conv (k = 1, 2, 4) from pair rows into a
//                        channel slice of an fp32 NCHW map
// Both gather their A fragments straight into the MFMA operand layout (lane (r, h): row r, eight
// consecutive channels 8h .. 8h+7 of a 16-channel step) and read W's fragments from the packed
// [N][2][K] pair rows; three f16 MFMA passes lo*Whi + hi*Wlo + hi*Whi per step with fp32
// accumulation in fixed K order.  No atomics on the data path (one writer per element), no call
// synchronises with the host.
#include "cmt_common.h"

namespace {

constexpr int BEV_TM = 64;      // conv: output rows per workgroup (2 waves x 32)
constexpr int BEV_TN = 128;     // conv: output channels per workgroup (2 waves x 64)
constexpr int BEV_WMAX = 180;   // the widest map (the NCHW halo conv's limit, shared so a chain fits or not as a whole)
constexpr int BEV_DB_WAVES = 2; // deblock: waves per workgroup, 32 output channels each
constexpr int BEV_DB_TM = 32;   // deblock: input pixels per workgroup

__global__ __launch_bounds__(256) void bev_conv3x3_kernel(cmt_bev_conv_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int s = a.stride;
    const int Ho = (a.H - 1) / s + 1, Wo = (a.W - 1) / s + 1;
    const int M = a.B * Ho * Wo;
    const int row0 = blockIdx.x * BEV_TM + (wave & 1) * 32;
    if (row0 >= M) return;   // wave-uniform; the kernel has no barrier
    const int n0 = blockIdx.y * BEV_TN + (wave >> 1) * 64;
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
    const pair_t* X = (const pair_t*)a.X;
    const pair_t* w0 = (const pair_t*)a.Wt + (int64_t)(n0 + r) * a.ldw + 8 * h;
    const pair_t* w1 = w0 + 32 * a.ldw;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;

    for (int tap = 0; tap < 9; ++tap) {
        const int yi = yo * s - 1 + tap / 3, xi = xo * s - 1 + tap % 3;
        const bool ok = live && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
        if (__ballot(ok) == 0) continue;   // a tap that is padding for every row of the wave
        const pair_t* xr = X + ((int64_t)(b * a.H + (ok ? yi : 0)) * a.W + (ok ? xi : 0)) * a.ldx + 8 * h;
        for (int c = 0; c < Cin; c += 16) {
            pair8_t ahi, alo;
#pragma unroll
            for (int j = 0; j < 8; ++j) ahi[j] = alo[j] = (pair_t)0.f;
            if (ok) {
                ahi = *(const pair8_t*)(xr + c);
                alo = *(const pair8_t*)(xr + Cin + c);
            }
            const int k = tap * Cin + c;
            acc0 = mma3(ahi, alo, *(const pair8_t*)(w0 + k), *(const pair8_t*)(w0 + K + k), acc0);
            acc1 = mma3(ahi, alo, *(const pair8_t*)(w1 + k), *(const pair8_t*)(w1 + K + k), acc1);
        }
    }

    pair_t* Y = (pair_t*)a.Y;
    bool bad = false;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int col = n0 + nb * 32 + r;
        const float sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + acc_row(i, h);
            if (row >= M) continue;
            float v = (nb ? acc1[i] : acc0[i]) + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            store_pair(Y + (int64_t)row * a.ldy, a.Cout, col, v);
        }
    }
    raise_range_flag(a.range_flag, bad);
}

// One workgroup: BEV_DB_TM input pixels x (BEV_DB_WAVES x 32) output channels x one dy x all KK dx.
// A wave's KK accumulators are staged through LDS as tile[n][KK * pixel + dx] (column index XORed
// with n: conflict-free for the column-wise writes and the row-wise reads), then stored as runs
// along x of the NCHW output.
template <int KK>
__global__ __launch_bounds__(64 * BEV_DB_WAVES) void bev_deblock_kernel(cmt_bev_deblock_args a) {
    constexpr int TW = BEV_DB_TM * KK;   // staged floats per channel
    __shared__ float s_tile[BEV_DB_WAVES][32][TW];
    __shared__ int64_t s_pix[BEV_DB_TM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int M = a.B * a.H * a.W;
    const int row0 = blockIdx.x * BEV_DB_TM;       // < M by the grid
    const int n0 = (blockIdx.y * BEV_DB_WAVES + wave) * 32;
    const int dy = blockIdx.z;
    const int Hout = KK * a.H, Wout = KK * a.W;
    if (threadIdx.x < BEV_DB_TM) {
        const int m = row0 + threadIdx.x;
        int64_t off = -1;
        if (m < M) {
            const int b = m / (a.H * a.W);
            const int p = m - b * (a.H * a.W);
            const int y = p / a.W, x = p - y * a.W;
            off = (((int64_t)b * a.Ctot + a.c0) * Hout + (KK * y + dy)) * Wout + KK * x;
        }
        s_pix[threadIdx.x] = off;
    }
    const int m = row0 + r;
    const bool live = m < M;
    const int Cin = a.Cin;
    const pair_t* xr = (const pair_t*)a.X + (int64_t)(live ? m : 0) * a.ldx + 8 * h;
    const pair_t* wr = (const pair_t*)a.Wt + ((int64_t)(dy * KK) * a.Cout + n0 + r) * a.ldw + 8 * h;
    f32x16 acc[KK];
#pragma unroll
    for (int d = 0; d < KK; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[d][i] = 0.f;
    for (int c = 0; c < Cin; c += 16) {
        pair8_t ahi, alo;
#pragma unroll
        for (int j = 0; j < 8; ++j) ahi[j] = alo[j] = (pair_t)0.f;
        if (live) {
            ahi = *(const pair8_t*)(xr + c);
            alo = *(const pair8_t*)(xr + Cin + c);
        }
#pragma unroll
        for (int d = 0; d < KK; ++d) {
            const pair_t* w = wr + (int64_t)d * a.Cout * a.ldw + c;
            acc[d] = mma3(ahi, alo, *(const pair8_t*)w, *(const pair8_t*)(w + Cin), acc[d]);
        }
    }
    const float sh = a.shift[n0 + r];
    bool bad = false;
#pragma unroll
    for (int d = 0; d < KK; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = acc_row(i, h);
            float v = acc[d][i] + sh;
            bad |= (row0 + p < M) && f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            s_tile[wave][r][(KK * p + d) ^ r] = v;
        }
    raise_range_flag(a.range_flag, bad);
    __syncthreads();
    const int64_t plane = (int64_t)Hout * Wout;
    for (int e = lane; e < 32 * TW; e += 64) {
        const int n = e / TW, j = e - n * TW;
        const int64_t off = s_pix[j / KK];
        if (off >= 0) a.Y[off + (int64_t)(n0 + n) * plane + (j % KK)] = s_tile[wave][n][j ^ n];
    }
}

}  // namespace

extern "C" int64_t cmt_bev_conv_args_size(void) { return (int64_t)sizeof(cmt_bev_conv_args); }
extern "C" int64_t cmt_bev_deblock_args_size(void) { return (int64_t)sizeof(cmt_bev_deblock_args); }

extern "C" int cmt_bev_conv3x3(const cmt_bev_conv_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_bev_conv3x3: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->Y, "cmt_bev_conv3x3: X, Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_bev_conv3x3: B, H and W must be positive");
    CMT_REQUIRE(a->stride == 1 || a->stride == 2, "cmt_bev_conv3x3: stride must be 1 or 2");
    CMT_REQUIRE(a->Cin > 0 && a->Cin % 32 == 0, "cmt_bev_conv3x3: Cin must be a positive multiple of 32");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % BEV_TN == 0, "cmt_bev_conv3x3: Cout must be a positive multiple of 128");
    CMT_REQUIRE(a->W <= BEV_WMAX, "cmt_bev_conv3x3: map width above 180");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_bev_conv3x3: B*H*W must be below 2^31");
    CMT_REQUIRE(a->ldx >= 2 * (int64_t)a->Cin && a->ldx % 8 == 0 && a->ldw >= 18 * (int64_t)a->Cin && a->ldw % 8 == 0 &&
                    a->ldy >= 2 * (int64_t)a->Cout,
                "cmt_bev_conv3x3: ldx >= 2 Cin, ldw >= 18 Cin (both % 8, 16-bit words) and ldy >= 2 Cout required");
    CMT_REQUIRE(aligned16(a->X) && aligned16(a->Wt), "cmt_bev_conv3x3: X and Wt must be 16-byte aligned");
    const int s = a->stride;
    const int64_t M = (int64_t)a->B * ((a->H - 1) / s + 1) * ((a->W - 1) / s + 1);
    dim3 grid((unsigned)cdiv64(M, BEV_TM), (unsigned)(a->Cout / BEV_TN));
    bev_conv3x3_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch("cmt_bev_conv3x3");
}

extern "C" int cmt_bev_deblock(const cmt_bev_deblock_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_bev_deblock: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->Y, "cmt_bev_deblock: X, Wt, shift and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_bev_deblock: B, H and W must be positive");
    CMT_REQUIRE(a->k == 1 || a->k == 2 || a->k == 4, "cmt_bev_deblock: k must be 1, 2 or 4");
    CMT_REQUIRE(a->Cin > 0 && a->Cin % 32 == 0, "cmt_bev_deblock: Cin must be a positive multiple of 32");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % 128 == 0, "cmt_bev_deblock: Cout must be a positive multiple of 128");
    CMT_REQUIRE(a->c0 >= 0 && (int64_t)a->c0 + a->Cout <= a->Ctot, "cmt_bev_deblock: slice [c0, c0 + Cout) outside Ctot");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_bev_deblock: B*H*W must be below 2^31");
    CMT_REQUIRE(a->ldx >= 2 * (int64_t)a->Cin && a->ldx % 8 == 0 && a->ldw >= 2 * (int64_t)a->Cin && a->ldw % 8 == 0,
                "cmt_bev_deblock: ldx, ldw >= 2 Cin and % 8 (16-bit words) required");
    CMT_REQUIRE(aligned16(a->X) && aligned16(a->Wt), "cmt_bev_deblock: X and Wt must be 16-byte aligned");
    const int64_t M = (int64_t)a->B * a->H * a->W;
    dim3 grid((unsigned)cdiv64(M, BEV_DB_TM), (unsigned)(a->Cout / (32 * BEV_DB_WAVES)), (unsigned)a->k);
    hipStream_t s = (hipStream_t)stream;
    switch (a->k) {
        case 1: bev_deblock_kernel<1><<<grid, 64 * BEV_DB_WAVES, 0, s>>>(*a); break;
        case 2: bev_deblock_kernel<2><<<grid, 64 * BEV_DB_WAVES, 0, s>>>(*a); break;
        default: bev_deblock_kernel<4><<<grid, 64 * BEV_DB_WAVES, 0, s>>>(*a); break;
    }
    return cmt_check_launch("cmt_bev_deblock");
}
