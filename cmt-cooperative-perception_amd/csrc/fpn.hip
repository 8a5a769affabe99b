// Camera neck kernels (the FPN over the image backbone's maps, mmdet's CPFPN), declared in
// include/cmt_hip.h (cmt_fpn_lateral, cmt_rows_to_nchw):
//   fpn_lateral_kernel    1 x 1 conv read transposed from the fp32 NCHW map, the coarser level's
//                         nearest-upsampled pair rows added in the epilogue, to CMT_F16P rows
//   rows_to_nchw_kernel   pair rows (or plain fp16 rows) -> fp32 NCHW through a 64 x 64 LDS transpose
// The lateral gathers its A fragments straight into the MFMA operand layout (lane (r, h): pixel r,
// channels 8h .. 8h+7 of a 16-channel step, one coalesced dword load per channel) and splits them in
// registers; W's fragments come from the packed [N][2][K] pair rows through LDS; three f16 MFMA passes
// lo*Whi + hi*Wlo + hi*Whi per step with fp32 accumulation in fixed K order.  No atomics on the data
// path (one writer per element), no call synchronises with the host.
#include <math.h>

#include "cmt_common.h"

namespace {

constexpr int FPN_TM = 128;     // lateral: pixels per workgroup (4 waves x 32), all of one image
constexpr int FPN_TN = 128;     // lateral: output channels per workgroup
constexpr int FPN_KC = 64;      // lateral: k per staged chunk of W (four 16-k steps, one 128-byte line per row half)
constexpr int FPN_WROW = 128;   // lateral: 16-bit words per LDS row of a W chunk (hi 64 | lo 64)
constexpr int FPN_XCDS = 8;   // workgroups are dealt round-robin over this many L2 domains

// torch's nearest source index for F.interpolate(size=...): one fp32 multiply by in / out
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    return min((int)floorf((float)dst * scale), in_size - 1);
}

// One workgroup: 128 pixels of one image (4 waves x 32) x 128 output channels (every wave all of them).
// A pixel tile lies inside one image (tile -> (b, first pixel)), so its channel loads never run into
// the next image's planes.  Each wave loads its own 32 pixels x 16 channels of X straight into the A
// fragment, four steps ahead.  W goes through LDS in chunks of 64 k (four steps), double-buffered, one
// barrier per chunk: a row's hi or lo half of a chunk is one 128-byte line, read by 8 adjacent lanes,
// 16 bytes each, two pieces per thread and step, issued two chunks ahead and written one chunk ahead.
// LDS rows are 256 bytes (hi 64 | lo 64) with the 16-byte piece index XORed with row % 16: the 16 rows a
// ds_read_b128 serves in one cycle, and the 8 pieces a ds_write_b128 does, fall on distinct banks.
// The workgroups that share a pixel tile (one per 128 output channels) sit next to each other in the same
// L2 domain: id -> (domain id % 8, slot id / 8), slot -> (channel group, tile), so X comes from HBM once.
__global__ __launch_bounds__(256) void fpn_lateral_kernel(cmt_fpn_lateral_args a, float scale_h, float scale_w,
                                                          int tiles_per_img, int ntiles) {
    __shared__ __attribute__((aligned(16))) pair_t s_w[2][FPN_TN * FPN_WROW];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int groups = a.Cout / FPN_TN;
    const int slot = blockIdx.x / FPN_XCDS;
    const int tile = (slot / groups) * FPN_XCDS + (blockIdx.x % FPN_XCDS);
    if (tile >= ntiles) return;   // workgroup-uniform
    const int b = tile / tiles_per_img;
    const int HW = a.H * a.W;
    const int tile_p0 = (tile - b * tiles_per_img) * FPN_TM;   // < HW by the grid
    const int p0 = tile_p0 + wave * 32;
    const int n0 = (slot % groups) * FPN_TN;
    const bool live = p0 + r < HW;
    const int Cin = a.Cin;
    const int nsteps = Cin / 16;
    // a lane past the image reads the tile's first pixel (its products land in rows that are never stored);
    // such a wave still takes part in the staging of W and in the barriers
    const float* xp = a.X + (int64_t)b * a.x_bstride + (int64_t)(8 * h) * HW + (live ? p0 + r : tile_p0);
    // W piece (j, i) of this thread in a chunk, j the step it is issued in, i = 0, 1: row (t >> 4) + 16 (2j + i),
    // hi / lo (t >> 3) % 2, k = 8 (t % 8) .. + 7 of the chunk.  Past Cin the k offset repeats the last piece
    // (min): never used, and every step issues the same loads, so the waits stay counted.
    const int wpart = (t >> 3) & 1;
    const pair_t* wsrc = (const pair_t*)a.Wt + (int64_t)(n0 + (t >> 4)) * a.ldw + wpart * Cin;
    const int64_t wstep = 16 * a.ldw;
    const int wdst = (t >> 4) * FPN_WROW + (((8 * wpart + (t & 7)) ^ (t >> 4)) * 8);
    const int wk = 8 * (t & 7);
    f32x16 acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[f][i] = 0.f;

    // Ring slot j holds step 4m + j's X, and the W pieces (j, .) of chunk m + 1 until step 4m + j writes them
    // to the other buffer and refills the slot with chunk m + 2's (W first, so the wait for a W piece never
    // waits for a younger X load).  The twelve MFMAs of a step run pass by pass; each accumulator sums
    // lo*Whi, hi*Wlo, hi*Whi in that order.
    bool bad = false;
    float xq[4][8];
    pair8_t wq[4][2];
    {
        const int k0 = min(wk, Cin - 8), k1 = min(FPN_KC + wk, Cin - 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                *(pair8_t*)&s_w[0][wdst + 16 * (2 * j + i) * FPN_WROW] = *(const pair8_t*)(wsrc + (2 * j + i) * wstep + k0);
                wq[j][i] = *(const pair8_t*)(wsrc + (2 * j + i) * wstep + k1);
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 16 * min(j, nsteps - 1);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) xq[j][jj] = xp[(int64_t)(c + jj) * HW];
        }
    }
    __syncthreads();
    // W fragments of step (m, j) from buffer m % 2: lane (r, h) of fragment f holds row 32f + r, k = 16j + 8h .. + 7
    auto read_b = [&](const pair_t* buf, int j, pair8_t* bhi, pair8_t* blo) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const pair_t* row = buf + (32 * f + r) * FPN_WROW;
            bhi[f] = *(const pair8_t*)(row + (((2 * j + h) ^ (r & 15)) * 8));
            blo[f] = *(const pair8_t*)(row + (((8 + 2 * j + h) ^ (r & 15)) * 8));
        }
    };
    pair8_t bhi[4], blo[4], nhi[4], nlo[4];
    read_b(s_w[0], 0, bhi, blo);
    for (int m = 0; 4 * m < nsteps; ++m) {
        const pair_t* rd = s_w[m & 1];
        pair_t* wr = s_w[(m + 1) & 1];
        const int k2 = min(FPN_KC * (m + 2) + wk, Cin - 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = 4 * m + j;
            if (s >= nsteps) break;   // workgroup-uniform
            pair8_t ahi, alo;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                bad |= f16_unrepresentable(xq[j][jj]);
                pair_t hi, lo;
                split_pair(xq[j][jj], hi, lo);
                ahi[jj] = hi;
                alo[jj] = lo;
            }
            // the next step's fragments come in under this step's MFMAs (the next chunk's first: after the barrier)
            if (j < 3) read_b(rd, j + 1, nhi, nlo);
            // the other buffer was last read before the barrier that ended chunk m - 1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                *(pair8_t*)&wr[wdst + 16 * (2 * j + i) * FPN_WROW] = wq[j][i];
                wq[j][i] = *(const pair8_t*)(wsrc + (2 * j + i) * wstep + k2);
            }
            const int c = 16 * min(s + 4, nsteps - 1);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) xq[j][jj] = xp[(int64_t)(c + jj) * HW];
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi[f], acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo[f], acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi[f], acc[f], 0, 0, 0);
            if (j < 3) {
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    bhi[f] = nhi[f];
                    blo[f] = nlo[f];
                }
            }
        }
        __syncthreads();
        read_b(wr, 0, bhi, blo);   // past the last chunk: read and never used
    }
    bad &= live;

    const pair_t* T = (const pair_t*)a.T;
    pair_t* L = (pair_t*)a.L;
    float sh[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) sh[f] = a.shift[n0 + 32 * f + r];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = p0 + acc_row(i, h);
        if (p >= HW) continue;
        float v[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            v[f] = acc[f][i] + sh[f];
            bad |= f16_unrepresentable(v[f]);
            if (a.relu) v[f] = fmaxf(v[f], 0.f);
        }
        if (T != nullptr) {
            const int y = p / a.W, x = p - y * a.W;
            const int sy = nearest_src(y, scale_h, a.Htop), sx = nearest_src(x, scale_w, a.Wtop);
            const pair_t* t = T + ((int64_t)(b * a.Htop + sy) * a.Wtop + sx) * a.ldt + n0 + r;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                v[f] += (float)t[32 * f] + (float)t[a.Cout + 32 * f];
                bad |= f16_unrepresentable(v[f]);
            }
        }
        pair_t* row = L + ((int64_t)b * HW + p) * a.ldl;
#pragma unroll
        for (int f = 0; f < 4; ++f) store_pair(row, a.Cout, n0 + 32 * f + r, v[f]);
    }
    raise_range_flag(a.range_flag, bad);
}

// One workgroup: 64 pixels x 64 channels of one image.  Loads are 16 bytes along channels (8 lanes per
// pixel row): of hi and of lo from pair rows (WORDS 2), or one of plain fp16 rows [B*HW][C] widened exactly
// (WORDS 1, the image backbone's one-pass policy).  Stores run along pixels: 16 bytes per lane where
// HW % 4 == 0 (VEC), 4 bytes otherwise.  LDS tile [64 c][65]: bank (c + p) % 64, conflict-free for both
// store forms.
template <int WORDS, bool VEC>
__global__ __launch_bounds__(256) void rows_to_nchw_kernel(cmt_rows_to_nchw_args a) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int C = a.C, HW = a.HW;
    {
        const int cg = (t & 7) * 8, pl = t >> 3;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int pi = pass * 32 + pl;
            if (p0 + pi < HW && c0 + cg < C) {
                const pair_t* row = (const pair_t*)a.X + ((int64_t)b * HW + p0 + pi) * a.ldx + c0 + cg;
                const pair8_t hi = *(const pair8_t*)row;
                if constexpr (WORDS == 2) {
                    const pair8_t lo = *(const pair8_t*)(row + C);
#pragma unroll
                    for (int j = 0; j < 8; ++j) tile[cg + j][pi] = (float)hi[j] + (float)lo[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) tile[cg + j][pi] = (float)hi[j];
                }
            }
        }
    }
    __syncthreads();
    float* Y = a.Y + (int64_t)b * C * HW;
    if constexpr (VEC) {
        const int q = (t & 15) * 4, cr = t >> 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + cr + 16 * k, p = p0 + q;
            if (c < C && p < HW) {   // HW % 4 == 0: the four pixels are inside together
                const float* s = &tile[cr + 16 * k][q];
                *(f32x4*)(Y + (int64_t)c * HW + p) = f32x4{s[0], s[1], s[2], s[3]};
            }
        }
    } else {
        const int px = t & 63, cr = t >> 6;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = c0 + cr + 4 * k;
            if (c < C && p0 + px < HW) Y[(int64_t)c * HW + p0 + px] = tile[cr + 4 * k][px];
        }
    }
}

}  // namespace

extern "C" int64_t cmt_fpn_lateral_args_size(void) { return (int64_t)sizeof(cmt_fpn_lateral_args); }
extern "C" int64_t cmt_rows_to_nchw_args_size(void) { return (int64_t)sizeof(cmt_rows_to_nchw_args); }

extern "C" int cmt_fpn_lateral(const cmt_fpn_lateral_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_fpn_lateral: null argument struct");
    CMT_REQUIRE(a->X && a->Wt && a->shift && a->L, "cmt_fpn_lateral: X, Wt, shift and L must be non-null");
    CMT_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "cmt_fpn_lateral: B, H and W must be positive");
    CMT_REQUIRE(a->Cin > 0 && a->Cin % 16 == 0, "cmt_fpn_lateral: Cin must be a positive multiple of 16");
    CMT_REQUIRE(a->Cout > 0 && a->Cout % FPN_TN == 0, "cmt_fpn_lateral: Cout must be a positive multiple of 128");
    CMT_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "cmt_fpn_lateral: B*H*W must be below 2^31");
    const int64_t HW = (int64_t)a->H * a->W;
    CMT_REQUIRE(a->x_bstride >= (int64_t)a->Cin * HW, "cmt_fpn_lateral: x_bstride below Cin*H*W");
    CMT_REQUIRE(a->ldw >= 2 * (int64_t)a->Cin && a->ldw % 8 == 0 && a->ldl >= 2 * (int64_t)a->Cout && a->ldl % 8 == 0,
                "cmt_fpn_lateral: ldw >= 2 Cin and ldl >= 2 Cout, both % 8 (16-bit words), required");
    CMT_REQUIRE(aligned16(a->Wt) && aligned16(a->L), "cmt_fpn_lateral: Wt and L must be 16-byte aligned");
    float scale_h = 0.f, scale_w = 0.f;
    if (a->T != nullptr) {
        CMT_REQUIRE(a->Htop >= 1 && a->Htop <= a->H && a->Wtop >= 1 && a->Wtop <= a->W,
                    "cmt_fpn_lateral: 1 <= Htop <= H and 1 <= Wtop <= W required with T");
        CMT_REQUIRE(a->ldt >= 2 * (int64_t)a->Cout && a->ldt % 8 == 0 && aligned16(a->T),
                    "cmt_fpn_lateral: ldt >= 2 Cout, % 8, and a 16-byte aligned T required");
        scale_h = (float)a->Htop / (float)a->H;
        scale_w = (float)a->Wtop / (float)a->W;
    }
    const int64_t tiles_per_img = cdiv64(HW, FPN_TM);
    const int64_t ntiles = a->B * tiles_per_img;
    const int64_t blocks = cdiv64(ntiles, FPN_XCDS) * FPN_XCDS * (a->Cout / FPN_TN);
    CMT_REQUIRE(blocks < ((int64_t)1 << 31), "cmt_fpn_lateral: grid too large");
    fpn_lateral_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, scale_h, scale_w, (int)tiles_per_img,
                                                                              (int)ntiles);
    return cmt_check_launch("cmt_fpn_lateral");
}

template <int WORDS>
static int rows_to_nchw(const char* name, const cmt_rows_to_nchw_args* a, void* stream) {
    const std::string n = std::string(name) + ": ";
    CMT_REQUIRE(a != nullptr, n + "null argument struct");
    CMT_REQUIRE(a->X && a->Y, n + "X and Y must be non-null");
    CMT_REQUIRE(a->B > 0 && a->HW > 0, n + "B and HW must be positive");
    CMT_REQUIRE(a->C > 0 && a->C % 8 == 0, n + "C must be a positive multiple of 8");
    CMT_REQUIRE(a->B <= 65535 && a->C <= 65535 * 64, n + "B or C beyond the grid");
    CMT_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), n + "B*HW must be below 2^31");
    CMT_REQUIRE(a->ldx >= WORDS * (int64_t)a->C && a->ldx % 8 == 0 && aligned16(a->X),
                n + (WORDS == 2 ? "ldx >= 2 C" : "ldx >= C") + ", % 8 (16-bit words), and a 16-byte aligned X required");
    CMT_REQUIRE((((uintptr_t)a->Y) & 3) == 0, n + "Y must be 4-byte aligned");
    dim3 grid((unsigned)cdiv(a->HW, 64), (unsigned)cdiv(a->C, 64), (unsigned)a->B);
    if (a->HW % 4 == 0 && aligned16(a->Y))
        rows_to_nchw_kernel<WORDS, true><<<grid, 256, 0, (hipStream_t)stream>>>(*a);
    else
        rows_to_nchw_kernel<WORDS, false><<<grid, 256, 0, (hipStream_t)stream>>>(*a);
    return cmt_check_launch(name);
}

extern "C" int cmt_rows_to_nchw(const cmt_rows_to_nchw_args* a, void* s) { return rows_to_nchw<2>("cmt_rows_to_nchw", a, s); }
extern "C" int cmt_rows_to_nchw_f16(const cmt_rows_to_nchw_args* a, void* s) { return rows_to_nchw<1>("cmt_rows_to_nchw_f16", a, s); }
