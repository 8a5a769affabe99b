// Linear -> ReLU -> Linear in one launch at the reference's fp32 numerics
// (cmt_mlp2_x3, cmt_hip.h): the camera position encoder rv_embedding
// (cmt_head.py:297-301) over the frustum coordinates of _rv_pe (cmt_head.py:
// 417-433, 24 000 rows per nuScenes frame) and the query coordinates of
// _rv_query_embed (cmt_head.py:439-467).
//
// The two-GEMM form writes the 1024-wide hidden activation as f16 pairs to HBM
// (98 MB per frame) and reads it back; its short-K first GEMM (K = 192, six
// k-stages per tile) is pipeline fill and epilogue, its 256-column second GEMM
// covers 188 tiles of a 256-CU chip.  Here one wave owns 32 rows end to end:
//
//   A fragments (its rows, all K) stay in registers for the whole launch;
//   for each 32-unit hidden block hb:
//     H^T[hb] = W1[hb] . A^T            (swapped 32x32x16 form: lane = row,
//                                        registers = hidden units)
//     H = relu(H + b1) split into f16 hi / lo in registers
//     OUT^T += W2[:, hb] . H^T          (H^T's registers are the B operand: the
//                                        pack orders W2's k like them, so the
//                                        hidden tile never leaves the wave)
//
// Every product is the three-pass split-f16 product of cmt_gemm (W_hi A_lo +
// W_lo A_hi + W_hi A_hi, fp32 accumulation); fc1 runs cmt_gemm's k order, so H
// equals the two-GEMM path's hidden values bit for bit.  The weights of a hidden
// block (W1: K/16 x 2 KB, W2: 32 KB) are shared by the workgroup's 4 waves
// through LDS: a two-slot ring per matrix filled by LDS-DMA one block ahead, one
// barrier per block, and the MFMAs of fc2(hb) interleaved with those of
// fc1(hb + 1) (independent accumulators).  Each wave issues its DMA pieces one
// per MFMA step in the first half of a block, behind that step's MFMAs (issued
// as a burst after the barrier they idled the matrix pipe: 95 -> 89 us for the
// fused camera rows, profiles/r6_experiments.txt r6j).  One wave per SIMD: the 8 output
// accumulator tiles (128 registers), the A fragments (96 at K = 192) and the
// hidden tile need the whole 512-register file.
//
// The camera rows' default form is cmt_mlp2_affine (mlp2_affine_kernel below): the frustum
// coordinates are affine in the pixel, so fc1 over them is two FMAs per hidden unit with
// per-camera coefficients and only fc2 runs on the matrix pipe; the epilogues are shared.
#include "cmt_common.h"

#include <type_traits>

namespace {

constexpr int MW = 4;               // waves per workgroup, one per SIMD
constexpr int MROWS = 32 * MW;      // rows per workgroup
constexpr int NOUT = 256;           // output width
constexpr int NOT = NOUT / 32;      // output tiles per wave
constexpr int FRAG_B = 1024;        // one fragment image: 64 lanes x 16 bytes
constexpr int W2_BLK = NOT * 2 * 2 * FRAG_B;   // one hidden block of W2p: 32 KB
constexpr int MAX_HD = 2048;
        // hidden width bound (b1 staged in LDS)

__device__ __forceinline__ f32x16 mma3(const pair8_t& wh, const pair8_t& wl, const pair8_t& xh, const pair8_t& xl,
                                       f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc, 0, 0, 0);
}

#ifndef CMT_MLP_DIAG
#define CMT_MLP_DIAG 0   // dev diagnostics (wrong results): 1 no C2 stores, 2 no NCHW loads, 4 no coordinates,
                         // 8 no weight DMA after the prologue
#endif

// ---- the epilogues, shared by the GEMM form (mlp2_x3_kernel) and the affine form
// (mlp2_affine_kernel).  Both hold the output as oacc[ot][4 g + e]: row lr = lane & 31, column
// 32 ot + 8 g + 4 lh + e (lh = lane >> 5).

// RX: the 256 NCHW feature values of the lane's row (view image gimg, pixel gpix of ghw)
__device__ __forceinline__ void rx_load(const cmt_mlp2_args& a, int gimg, int gpix, int ghw, int lh,
                                        float (&xv)[4][2][4][4]) {
    const float* const xrow = a.rx + (int64_t)gimg * NOUT * ghw + gpix;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    xv[q][tt][g][e] = (CMT_MLP_DIAG & 2) ? 0.f
                                                         : xrow[(int64_t)((2 * q + tt) * 32 + 8 * g + 4 * lh + e) * ghw];
}
__device__ __forceinline__ void rx_load(const cmt_mlp2_args&, int, int, int, int, float (&)[1][2][4][4]) {}

// The fused camera rows: the memory-row pair (C2) from the NCHW features and
// out = acc + (b2 + pair value) (C), both staged through LDS per column quarter so every
// global store is 16 contiguous bytes of a 128-byte row segment (8 lanes per row).  lds: the
// workgroup's weight rings (at least 64 KB), which become the staging once every wave is past them
__device__ __forceinline__ void rx_epilogue(const cmt_mlp2_args& a, char* lds, const f32x16 (&oacc)[NOT],
                                            const float (&xv)[4][2][4][4]) {
    const int lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int z = blockIdx.y;
    __syncthreads();   // every wave is past its last weight-ring read: the rings become staging
    char* const stg = lds + wave * 16384;            // 4 slices [32 rows][64 cols] f16: C hi / lo, C2 hi / lo
    const int mw0 = blockIdx.x * MROWS + wave * 32;  // the wave's first row
    bool bad = false;
    typedef pair_t p4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    auto sw = [](int r, int c16) { return r * 128 + ((c16 ^ ((r >> 1) & 7)) << 4); };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ot = 2 * q + tt;
                const int n = ot * 32 + 8 * g + 4 * lh;
                const f32x4 bv = *(const f32x4*)(a.b2 + n);
                p4 h2, l2, hc, lc;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // the pair cmt_nchw_to_rows writes, and its value as the pair R row reads back
                    const float x = xv[q][tt][g][e];
                    bad |= f16_unrepresentable(x);
                    h2[e] = (pair_t)x;
                    l2[e] = (pair_t)(x - (float)h2[e]);
                    const float rv = (float)h2[e] + (float)l2[e];
                    const float v = oacc[ot][4 * g + e] + (bv[e] + rv);
                    hc[e] = (pair_t)v;
                    lc[e] = (pair_t)(v - (float)hc[e]);
                }
                const int off = sw(lr, 4 * tt + g) + 8 * lh;
                *(p4*)(stg + off) = hc;
                *(p4*)(stg + 4096 + off) = lc;
                *(p4*)(stg + 8192 + off) = h2;
                *(p4*)(stg + 12288 + off) = l2;
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 8 * i + (lane >> 3), ch = lane & 7;
            const int mr = mw0 + r;
            const int off = sw(r, ch);
            const u4 v0 = *(const u4*)(stg + off), v1 = *(const u4*)(stg + 4096 + off);
            const u4 v2 = *(const u4*)(stg + 8192 + off), v3 = *(const u4*)(stg + 12288 + off);
            if (mr < a.M && !(CMT_MLP_DIAG & 1)) {
                pair_t* cr = (pair_t*)a.C + (int64_t)z * a.c_bstride + (int64_t)mr * a.ldc + 64 * q + 8 * ch;
                pair_t* c2 = (pair_t*)a.C2 + (int64_t)z * a.c2_bstride + (int64_t)mr * a.ldc2 + 64 * q + 8 * ch;
                *(u4*)cr = v0;
                *(u4*)(cr + NOUT) = v1;
                *(u4*)c2 = v2;
                *(u4*)(c2 + NOUT) = v3;
            }
        }
    }
    raise_range_flag(a.range_flag, bad);
}
__device__ __forceinline__ void rx_epilogue(const cmt_mlp2_args&, char*, const f32x16 (&)[NOT],
                                            const float (&)[1][2][4][4]) {}

// out = acc + (b2 + R) (cmt_gemm's order) for row m (row = min(m, M - 1))
__device__ __forceinline__ void rows_epilogue(const cmt_mlp2_args& a, int m, int row, const f32x16 (&oacc)[NOT]) {
    const int lh = (threadIdx.x & 63) >> 5;
    const int z = blockIdx.y;
    if (m >= a.M) return;
    const char* Rrow = nullptr;
    if (a.R) {
        const int resz = a.r_dtype == CMT_F32 ? 4 : 2;
        Rrow = (const char*)a.R + ((int64_t)z * a.r_bstride + (int64_t)row * a.ldr) * resz;
    }
    const int cesz = a.c_dtype == CMT_F32 ? 4 : 2;
    char* Crow = (char*)a.C + ((int64_t)z * a.c_bstride + (int64_t)row * a.ldc) * cesz;
    typedef pair_t p4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int ot = 0; ot < NOT; ++ot)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = ot * 32 + 8 * g + 4 * lh;
            const f32x4 bv = *(const f32x4*)(a.b2 + n);
            f32x4 rv = {0.f, 0.f, 0.f, 0.f};
            if (Rrow) {
                if (a.r_dtype == CMT_F32) {
                    rv = *(const f32x4*)((const float*)Rrow + n);
                } else {
                    const p4 h = *(const p4*)((const pair_t*)Rrow + n);
                    const p4 l = *(const p4*)((const pair_t*)Rrow + NOUT + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) rv[e] = (float)h[e] + (float)l[e];
                }
            }
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = oacc[ot][4 * g + e] + (bv[e] + rv[e]);
            if (a.c_dtype == CMT_F32) *(f32x4*)((float*)Crow + n) = v;
            else store_pair4((pair_t*)Crow, NOUT, n, v);
        }
}

// KS = K / 16; PD = the LDS fragment prefetch distance in steps (3: same time, 4: +8 %,
// profiles/r4t_mlp_prefetch.txt)
// GEO / RX (ABI 20): the frustum coordinates generated in the prologue and the residual read
// from the NCHW image features in the epilogue (cmt_hip.h cmt_mlp2_args.geo_i2l / rx)
template <int KS, int PD = 2, bool GEO = false, bool RX = false>
__global__ __launch_bounds__(64 * MW, 1) void mlp2_x3_kernel(cmt_mlp2_args a) {
    constexpr int W1_BLK = KS * 2 * FRAG_B;
    __shared__ __attribute__((aligned(16))) char lds[2 * W1_BLK + 2 * W2_BLK + MAX_HD * 4 + (GEO ? 64 * 4 : 0)];
    char* const s1 = lds;                 // W1 ring: 2 x W1_BLK
    char* const s2 = lds + 2 * W1_BLK;    // W2 ring: 2 x W2_BLK
    float* const sb1 = (float*)(lds + 2 * W1_BLK + 2 * W2_BLK);   // b1 (a global load per block
                                                                  // cost a memory round trip each)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int z = blockIdx.y;
    const int m = blockIdx.x * MROWS + wave * 32 + lr;
    const int row = min(m, a.M - 1);
    const int nhb = a.Hd / 32;
    const char* const w1g = (const char*)a.W1p;
    const char* const w2g = (const char*)a.W2p;

    // LDS-DMA of hidden block hb's fragments: piece p of a matrix by wave p % MW
    auto issue_w1 = [&](int hb) {
        if (hb >= nhb) return;
        const char* src = w1g + (int64_t)hb * W1_BLK + lane * 16;
        char* dst = s1 + (hb & 1) * W1_BLK;
#pragma unroll
        for (int p = wave; p < 2 * KS; p += MW) glds16(src + p * FRAG_B, dst + p * FRAG_B);
    };
    auto issue_w2 = [&](int hb) {
        if (hb >= nhb) return;
        const char* src = w2g + (int64_t)hb * W2_BLK + lane * 16;
        char* dst = s2 + (hb & 1) * W2_BLK;
#pragma unroll
        for (int p = wave; p < 4 * NOT; p += MW) glds16(src + p * FRAG_B, dst + p * FRAG_B);
    };
    issue_w1(0);
    issue_w2(0);
    issue_w1(1);
    for (int i = tid; i < a.Hd / 4; i += 64 * MW) *(f32x4*)(sb1 + 4 * i) = *(const f32x4*)(a.b1 + 4 * i);

    // this lane's row of A as the B operand of fc1 (k = 16 ks + 8 lh + j), hi and lo planes
    pair8_t ah[KS], al[KS];
    const int ghw = GEO || RX ? a.geo_h * a.geo_w : 1;
    const int gview = row / ghw, gpix = row - gview * ghw;      // GEO / RX: view and pixel of the row
    const int gimg = z * (a.M / ghw) + gview;
    if constexpr (GEO && (CMT_MLP_DIAG & 4)) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { ah[ks] = pair8_t{}; al[ks] = pair8_t{}; }
    } else if constexpr (GEO) {
        // rv_pe_coords_kernel8's arithmetic (elementwise.hip), element k = 3 depth + coordinate.
        // Element 16 ks + 8 lh + j is coordinate (ks + 2 lh + j) mod 3: with the matrix rows and
        // the range rotated by 2 lh once per lane, the row index (ks + j) mod 3 is a compile-time
        // constant (a lane-divergent register-array index is a waterfall loop); the depth values
        // d (one fp32 division each) come from an LDS table the workgroup fills first
        const int gw = gpix % a.geo_w, gh = gpix / a.geo_w;
        const float u = (float)gw * a.geo_pad_w / (float)a.geo_w;
        const float v = (float)gh * a.geo_pad_h / (float)a.geo_h;
        const float* Mx = a.geo_i2l + (int64_t)gimg * 16;
        float mr[3][4], plo[3], pspan[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int src0 = q, src1 = (q + 2) % 3;        // lh = 0 / lh = 1
#pragma unroll
            for (int i = 0; i < 4; ++i) mr[q][i] = lh ? Mx[src1 * 4 + i] : Mx[src0 * 4 + i];
            plo[q] = lh ? a.geo_pc[src1] : a.geo_pc[src0];
            pspan[q] = lh ? a.geo_pc[3 + src1] - a.geo_pc[src1] : a.geo_pc[3 + src0] - a.geo_pc[src0];
        }
        float* dtab = sb1 + MAX_HD;                         // 3 D depth values after b1 (KS * 16 / 3 <= 64)
        if (tid < a.geo_D) dtab[tid] = 1.f + (float)tid * (a.geo_depth_max - 1.f) / (float)a.geo_D;
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = 16 * ks + 8 * lh + j;
                const int r = (ks + j) % 3;                 // the rotated row: compile-time
                const float d = dtab[kk / 3];
                const float c0 = u * d, c1 = v * d;
                float s = mr[r][0] * c0;
                s = fmaf(mr[r][1], c1, s);
                s = fmaf(mr[r][2], d, s);
                s = fmaf(mr[r][3], 1.f, s);
                const float x = (s - plo[r]) / pspan[r];
                const pair_t h = (pair_t)x;
                ah[ks][j] = h;
                al[ks][j] = (pair_t)(x - (float)h);
            }
    } else {
        const pair_t* Ar = (const pair_t*)a.A + (int64_t)z * a.a_bstride + (int64_t)row * a.lda;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            ah[ks] = *(const pair8_t*)(Ar + 16 * ks + 8 * lh);
            al[ks] = *(const pair8_t*)(Ar + a.K + 16 * ks + 8 * lh);
        }
    }

    f32x16 oacc[NOT], hacc;
#pragma unroll
    for (int t = 0; t < NOT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    pair8_t hh[2], hl[2];   // the hidden tile as fc2's B operand (k-steps 0, 1), hi and lo

    // fc1 of block hb from its W1 slot into hacc
    auto fc1 = [&](int hb) {
        const char* w = s1 + (hb & 1) * W1_BLK + lane * 16;
#pragma unroll
        for (int r = 0; r < 16; ++r) hacc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const pair8_t wh = *(const pair8_t*)(w + (2 * ks) * FRAG_B);
            const pair8_t wl = *(const pair8_t*)(w + (2 * ks + 1) * FRAG_B);
            hacc = mma3(wh, wl, ah[ks], al[ks], hacc);
        }
    };
    // relu(hacc + b1) -> pairs; register r of lane half lh is hidden unit 8 (r >> 2) + 4 lh + (r & 3)
    auto split_hidden = [&](int hb) {
        const float* b1 = sb1 + hb * 32 + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 bv = *(const f32x4*)(b1 + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = fmaxf(hacc[4 * g + e] + bv[e], 0.f) + 0.f;
                const pair_t h = (pair_t)x;
                hh[g >> 1][4 * (g & 1) + e] = h;
                hl[g >> 1][4 * (g & 1) + e] = (pair_t)(x - (float)h);
            }
        }
    };
    // fc2 over block hb (its W2 slot), interleaved with fc1 of block hb + 1 when there is one.
    // Step t of the block's MFMA stream: with fc1, t < 2 KS alternates fc2 step t / 2 and fc1
    // step t / 2, then fc2 steps KS .. 15 follow; each step is a triple on one accumulator whose
    // two weight fragments (hi, lo) are read from LDS two steps ahead (a 3-slot register ring),
    // the order pinned by scheduling barriers -- left to itself the compiler read each pair right
    // before its MFMAs and waited for it (lgkmcnt(0)) 28 times per block.
    // this wave's j-th LDS-DMA piece of block hb's successors: W2(hb + 1) pieces first (needed from
    // the next block's first fc2 step), then W1(hb + 2)
    constexpr int NW2 = 4 * NOT / MW, NW1 = (2 * KS + MW - 1) / MW;
    auto dma_piece = [&](int hb, int j) {
        if (j < NW2) {
            if (hb + 1 >= nhb) return;
            const int p = wave + MW * j;
            glds16(w2g + (int64_t)(hb + 1) * W2_BLK + lane * 16 + p * FRAG_B,
                       s2 + ((hb + 1) & 1) * W2_BLK + p * FRAG_B);
        } else {
            const int p = wave + MW * (j - NW2);
            if (hb + 2 >= nhb || p >= 2 * KS) return;
            glds16(w1g + (int64_t)(hb + 2) * W1_BLK + lane * 16 + p * FRAG_B, s1 + (hb & 1) * W1_BLK + p * FRAG_B);
        }
    };
    auto fc2_fc1 = [&](int hb, auto next_c) {
        constexpr bool next = decltype(next_c)::value;   // compile-time: a branch-free MFMA stream
        constexpr int NSTEP = next ? 2 * NOT + KS : 2 * NOT;
        const char* w2 = s2 + (hb & 1) * W2_BLK + lane * 16;
        const char* w1 = s1 + ((hb + 1) & 1) * W1_BLK + lane * 16;
        auto is_fc2 = [](int t) { return !next || t >= 2 * KS || (t & 1) == 0; };
        auto index = [](int t) { return !next ? t : (t < 2 * KS ? t >> 1 : t - KS); };
        auto addr = [&](int t) { return (is_fc2(t) ? w2 : w1) + index(t) * 2 * FRAG_B; };
        if constexpr (next) {
#pragma unroll
            for (int r = 0; r < 16; ++r) hacc[r] = 0.f;
        }
        // fragments PD steps ahead (a register ring of PD + 1 slots)
        pair8_t fh[PD + 1], fl[PD + 1];
#pragma unroll
        for (int t = 0; t < PD; ++t) {
            fh[t] = *(const pair8_t*)addr(t);
            fl[t] = *(const pair8_t*)(addr(t) + FRAG_B);
        }
#pragma unroll
        for (int t = 0; t < NSTEP; ++t) {
            if (t + PD < NSTEP) {
                fh[(t + PD) % (PD + 1)] = *(const pair8_t*)addr(t + PD);
                fl[(t + PD) % (PD + 1)] = *(const pair8_t*)(addr(t + PD) + FRAG_B);
            }
            const int i = index(t);
            const int sl = t % (PD + 1);
            if (is_fc2(t)) oacc[i >> 1] = mma3(fh[sl], fl[sl], hh[i & 1], hl[i & 1], oacc[i >> 1]);
            else hacc = mma3(fh[sl], fl[sl], ah[i], al[i], hacc);
            // one weight piece per step behind the step's MFMAs (NW2 + NW1 <= NSTEP for every KS):
            // the wave issues its DMA while the matrix pipe is busy, half a block ahead of the wait
            if constexpr (next && !(CMT_MLP_DIAG & 8))
                if (t < NW2 + NW1) dma_piece(hb, t);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    barrier_mem();   // W1(0), W2(0), W1(1) landed for every wave's pieces
    fc1(0);
    split_hidden(0);
    for (int hb = 0; hb + 1 < nhb; ++hb) {
        // W2(hb) and W1(hb + 1) (issued one block ago) landed; every wave is past block hb - 1,
        // so the slots of W2(hb - 1) and W1(hb) take W2(hb + 1) and W1(hb + 2)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        barrier_mem();
        fc2_fc1(hb, std::true_type{});
        split_hidden(hb + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    barrier_mem();
    // RX: the row's 256 NCHW feature values are loaded here, into the registers fc1's A operand
    // held, so their memory round trip runs under the last block's fc2 instead of the epilogue's
    float xv[RX ? 4 : 1][2][4][4];
    if constexpr (RX) rx_load(a, gimg, gpix, ghw, lh, xv);
    fc2_fc1(nhb - 1, std::false_type{});   // the last block: fc2 only

    if constexpr (RX) rx_epilogue(a, lds, oacc, xv);
    else rows_epilogue(a, m, row, oacc);
}

// ---- the affine form (cmt_mlp2_affine, cmt_hip.h): the frustum coordinates are affine in the
// pixel and nothing nonlinear stands before fc1, so hidden unit j of a row of view b is
// relu(alpha_bj u + beta_bj v + gamma_bj): no fc1 GEMM, no coordinates.  The workgroup contracts
// the weight-only tables with the inverse camera matrices of the views its rows lie in (float64,
// rounded to fp32 into LDS); a wave's 32 rows lie in one view (h w % 32 == 0), so each hidden
// block's 16 coefficient triples per lane half are broadcast LDS reads.  fc2, the W2 ring and the
// epilogues are the GEMM form's.  The two FMAs and the pair split of block hb + 1's hidden tile
// run one unit per MFMA step inside block hb's fc2 stream, in the matrix pipe's shadow.
constexpr int AFF_MAX_HD = 1024;    // hidden width bound (coefficient tables in LDS)
constexpr int AFF_VIEWS = MROWS / 32;   // views a workgroup's rows can lie in

template <bool RX, int PD = 2>
__global__ __launch_bounds__(64 * MW, 1) void mlp2_affine_kernel(cmt_mlp2_affine_args aa) {
    const cmt_mlp2_args& a = aa.m;
    __shared__ __attribute__((aligned(16))) char lds[2 * W2_BLK + AFF_VIEWS * 3 * AFF_MAX_HD * 4];
    char* const s2 = lds;                                  // W2 ring: 2 x W2_BLK
    float* const sco = (float*)(lds + 2 * W2_BLK);         // [view slot][alpha, beta, gamma][AFF_MAX_HD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int z = blockIdx.y;
    const int m = blockIdx.x * MROWS + wave * 32 + lr;
    const int row = min(m, a.M - 1);
    const int nhb = a.Hd / 32;
    const char* const w2g = (const char*)a.W2p;
    const int ghw = a.geo_h * a.geo_w, nview = a.M / ghw;
    const int gview = row / ghw, gpix = row - gview * ghw;
    const int gimg = z * nview + gview;

    // W2(0): piece p by wave p % MW
#pragma unroll
    for (int p = wave; p < 4 * NOT; p += MW) glds16(w2g + lane * 16 + p * FRAG_B, s2 + p * FRAG_B);

    // the coefficients of the workgroup's views: alpha = sum_c T1[j][c] M[c][0], beta likewise with
    // M[c][1], gamma = sum_c (T1[j][c] M[c][2] + T0[j][c] (M[c][3] - lo_c)) + b0[j]
    const int v0 = blockIdx.x * MROWS / ghw;
    const int nv = min(blockIdx.x * MROWS + MROWS - 1, a.M - 1) / ghw - v0 + 1;   // <= AFF_VIEWS: h w >= 32
    for (int s = 0; s < nv; ++s) {
        const float* Mx = a.geo_i2l + (int64_t)(z * nview + v0 + s) * 16;
        double mm[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int i = 0; i < 3; ++i) mm[c][i] = (double)Mx[4 * c + i];
            mm[c][3] = (double)Mx[4 * c + 3] - (double)a.geo_pc[c];
        }
        // four units per thread and trip: their table loads are in flight together (one unit per
        // trip waited for each load, a memory round trip per 256 units)
#pragma unroll 4
        for (int j = tid; j < a.Hd; j += 64 * MW) {
            const double* t = aa.tab + 8 * j;
            double al = 0.0, be = 0.0, ga = t[6];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double t1 = t[c], t0 = t[3 + c];
                al = fma(t1, mm[c][0], al);
                be = fma(t1, mm[c][1], be);
                ga = fma(t1, mm[c][2], ga);
                ga = fma(t0, mm[c][3], ga);
            }
            float* o = sco + s * 3 * AFF_MAX_HD + j;
            o[0] = (float)al;
            o[AFF_MAX_HD] = (float)be;
            o[2 * AFF_MAX_HD] = (float)ga;
        }
    }
    const int gw = gpix % a.geo_w, gh = gpix / a.geo_w;
    const float u = (float)gw * a.geo_pad_w / (float)a.geo_w;
    const float v = (float)gh * a.geo_pad_h / (float)a.geo_h;
    const int slot = __builtin_amdgcn_readfirstlane(gview - v0);
    const float* const co = sco + slot * 3 * AFF_MAX_HD + 4 * lh;   // the lane half's alpha of unit 0

    f32x16 oacc[NOT];
#pragma unroll
    for (int t = 0; t < NOT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    // the hidden tile as fc2's B operand (k-steps 0, 1), hi and lo: this block's and the next one's.
    // Register 4 g + e of lane half lh is hidden unit 8 g + 4 lh + e, as in the GEMM form
    pair8_t hh[2], hl[2], nh[2], nl[2];
    f32x4 ca, cb, cc;
    auto coef_read = [&](int hb, int g) {
        const float* p = co + 32 * hb + 8 * g;
        ca = *(const f32x4*)p;
        cb = *(const f32x4*)(p + AFF_MAX_HD);
        cc = *(const f32x4*)(p + 2 * AFF_MAX_HD);
    };
    auto unit = [&](pair8_t (&H)[2], pair8_t (&L)[2], int g, int e) {
        const float x = fmaxf(fmaf(ca[e], u, fmaf(cb[e], v, cc[e])), 0.f) + 0.f;
        const pair_t h = (pair_t)x;
        H[g >> 1][4 * (g & 1) + e] = h;
        L[g >> 1][4 * (g & 1) + e] = (pair_t)(x - (float)h);
    };
    // fc2 over block hb (its W2 slot): 16 steps, each a triple on one accumulator whose two weight
    // fragments are read from LDS PD steps ahead.  With a next block, steps 0 .. 4 NOT / MW - 1 also
    // issue this wave's LDS-DMA pieces of W2(hb + 1), one per step behind the step's MFMAs, and
    // steps 4 g .. 4 g + 3 read group g's coefficients of block hb + 1 and form its four units
    constexpr int NW2 = 4 * NOT / MW;
    auto fc2 = [&](int hb, auto next_c) {
        constexpr bool next = decltype(next_c)::value;
        const char* w2 = s2 + (hb & 1) * W2_BLK + lane * 16;
        pair8_t fh[PD + 1], fl[PD + 1];
#pragma unroll
        for (int t = 0; t < PD; ++t) {
            fh[t] = *(const pair8_t*)(w2 + t * 2 * FRAG_B);
            fl[t] = *(const pair8_t*)(w2 + t * 2 * FRAG_B + FRAG_B);
        }
#pragma unroll
        for (int t = 0; t < 2 * NOT; ++t) {
            if constexpr (next)
                if (t % 4 == 0) coef_read(hb + 1, t / 4);
            if (t + PD < 2 * NOT) {
                fh[(t + PD) % (PD + 1)] = *(const pair8_t*)(w2 + (t + PD) * 2 * FRAG_B);
                fl[(t + PD) % (PD + 1)] = *(const pair8_t*)(w2 + (t + PD) * 2 * FRAG_B + FRAG_B);
            }
            const int sl = t % (PD + 1);
            oacc[t >> 1] = mma3(fh[sl], fl[sl], hh[t & 1], hl[t & 1], oacc[t >> 1]);
            if constexpr (next) {
                // the coefficients read at step 4 g are used from step 4 g + 1 on
                if (t % 4 >= 1) unit(nh, nl, t / 4, t % 4 - 1);
                if (t % 4 == 3) unit(nh, nl, t / 4, 3);
                if (t < NW2 && !(CMT_MLP_DIAG & 8)) {
                    const int p = wave + MW * t;
                    glds16(w2g + (int64_t)(hb + 1) * W2_BLK + lane * 16 + p * FRAG_B,
                           s2 + ((hb + 1) & 1) * W2_BLK + p * FRAG_B);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    barrier_mem();   // W2(0) landed for every wave's pieces, the coefficients are written
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        coef_read(0, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) unit(hh, hl, g, e);
    }
    for (int hb = 0; hb + 1 < nhb; ++hb) {
        // W2(hb) (issued one block ago) landed; every wave is past block hb - 1, whose slot takes
        // W2(hb + 1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        barrier_mem();
        fc2(hb, std::true_type{});
#pragma unroll
        for (int i = 0; i < 2; ++i) { hh[i] = nh[i]; hl[i] = nl[i]; }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    barrier_mem();
    // RX: the NCHW loads' memory round trip runs under the last block's fc2, as in the GEMM form
    float xv[RX ? 4 : 1][2][4][4];
    if constexpr (RX) rx_load(a, gimg, gpix, ghw, lh, xv);
    fc2(nhb - 1, std::false_type{});

    if constexpr (RX) rx_epilogue(a, lds, oacc, xv);
    else rows_epilogue(a, m, row, oacc);
}

// the checks of C and R both entry points share
int check_rows(const cmt_mlp2_args& a, const char* who) {
    const std::string w(who);
    CMT_REQUIRE(a.c_dtype == CMT_F32 || a.c_dtype == CMT_F16P, w + ": C must be fp32 or an f16 pair");
    CMT_REQUIRE(a.c_dtype == CMT_F32 ? a.ldc >= NOUT && a.ldc % 4 == 0 && a.c_bstride % 4 == 0
                                     : a.ldc >= 2 * NOUT && a.ldc % 4 == 0 && a.c_bstride % 4 == 0,
                w + ": bad C row stride");
    CMT_REQUIRE(a.R == nullptr || ((a.r_dtype == CMT_F32 && a.ldr >= NOUT) ||
                                   (a.r_dtype == CMT_F16P && a.ldr >= 2 * NOUT)) && a.ldr % 4 == 0 &&
                                      a.r_bstride % 4 == 0,
                w + ": R must be fp32 or f16-pair rows of 256");
    return 0;
}
// ... and of the fused camera-row outputs (rx, C2)
bool rx_ok(const cmt_mlp2_args& a) {
    return a.geo_i2l && a.rx && a.C2 && a.geo_h > 0 && a.geo_w > 0 && a.M % (a.geo_h * a.geo_w) == 0 &&
           a.c_dtype == CMT_F16P && a.R == nullptr && a.ldc2 >= 2 * NOUT && a.ldc2 % 4 == 0 &&
           a.c2_bstride % 4 == 0 && (uintptr_t)a.C2 % 8 == 0;
}

}  // namespace

extern "C" int64_t cmt_mlp2_args_size(void) { return (int64_t)sizeof(cmt_mlp2_args); }
extern "C" int64_t cmt_mlp2_affine_args_size(void) { return (int64_t)sizeof(cmt_mlp2_affine_args); }

extern "C" int cmt_mlp2_affine(const cmt_mlp2_affine_args* ap, void* stream) {
    CMT_REQUIRE(ap != nullptr, "cmt_mlp2_affine: null args");
    const cmt_mlp2_args& a = ap->m;
    CMT_REQUIRE(a.M > 0 && a.batch > 0, "cmt_mlp2_affine: empty problem");
    CMT_REQUIRE(a.N == NOUT, "cmt_mlp2_affine: the output width must be 256");
    CMT_REQUIRE(a.Hd > 0 && a.Hd % 32 == 0, "cmt_mlp2_affine: the hidden width must be a multiple of 32");
    CMT_REQUIRE(ap->tab && a.geo_i2l && a.W2p && a.b2 && a.C, "cmt_mlp2_affine: null pointer");
    CMT_REQUIRE(a.geo_h > 0 && a.geo_w > 0 && a.M % (a.geo_h * a.geo_w) == 0,
                "cmt_mlp2_affine: M must be a multiple of geo_h * geo_w");
    if (int rc = check_rows(a, "cmt_mlp2_affine")) return rc;
    CMT_REQUIRE(((uintptr_t)ap->tab | (uintptr_t)a.W2p | (uintptr_t)a.b2) % 16 == 0,
                "cmt_mlp2_affine: the tables, the pack and the bias must be 16-byte aligned");
    CMT_REQUIRE((a.rx == nullptr && a.C2 == nullptr) || rx_ok(a),
                "cmt_mlp2_affine: the fused camera-row form takes rx and C2 together, a pair C and no R");
    if (a.geo_h * a.geo_w % 32 != 0)
        return cmt_fail(CMT_ENOTSUP, "cmt_mlp2_affine: geo_h * geo_w must be a multiple of 32 (a wave's rows lie in "
                                     "one view)");
    if (a.Hd > AFF_MAX_HD) return cmt_fail(CMT_ENOTSUP, "cmt_mlp2_affine: the hidden width is at most 1024");
    const dim3 grid((unsigned)cdiv(a.M, MROWS), (unsigned)a.batch);
    hipStream_t s = (hipStream_t)stream;
    if (a.rx) mlp2_affine_kernel<true><<<grid, 64 * MW, 0, s>>>(*ap);
    else mlp2_affine_kernel<false><<<grid, 64 * MW, 0, s>>>(*ap);
    return cmt_check_launch("cmt_mlp2_affine");
}

extern "C" int cmt_mlp2_x3(const cmt_mlp2_args* ap, void* stream) {
    CMT_REQUIRE(ap != nullptr, "cmt_mlp2_x3: null args");
    const cmt_mlp2_args& a = *ap;
    CMT_REQUIRE(a.M > 0 && a.batch > 0, "cmt_mlp2_x3: empty problem");
    CMT_REQUIRE(a.N == NOUT, "cmt_mlp2_x3: the output width must be 256");
    CMT_REQUIRE(a.K > 0 && a.K % 16 == 0 && a.K <= 192, "cmt_mlp2_x3: K must be a multiple of 16, at most 192");
    CMT_REQUIRE(a.Hd > 0 && a.Hd % 32 == 0 && a.Hd <= MAX_HD,
                "cmt_mlp2_x3: the hidden width must be a multiple of 32, at most 2048");
    CMT_REQUIRE((a.A || a.geo_i2l) && a.W1p && a.W2p && a.b1 && a.b2 && a.C, "cmt_mlp2_x3: null pointer");
    CMT_REQUIRE(a.geo_i2l || (a.lda >= 2 * a.K && a.lda % 8 == 0 && a.a_bstride % 8 == 0),
                "cmt_mlp2_x3: A pair rows need lda >= 2K, 16-byte aligned");
    if (int rc = check_rows(a, "cmt_mlp2_x3")) return rc;
    CMT_REQUIRE(((uintptr_t)a.A | (uintptr_t)a.W1p | (uintptr_t)a.W2p) % 16 == 0 && (uintptr_t)a.b1 % 16 == 0 &&
                    (uintptr_t)a.b2 % 16 == 0,
                "cmt_mlp2_x3: A / packs / biases must be 16-byte aligned");
    const dim3 grid((unsigned)cdiv(a.M, MROWS), (unsigned)a.batch);
    hipStream_t s = (hipStream_t)stream;
    if (a.geo_i2l || a.rx) {
        CMT_REQUIRE(rx_ok(a) && a.K == 192 && a.geo_D * 3 == a.K,
                    "cmt_mlp2_x3: the fused camera-row form takes geo_i2l, rx and C2 together, K = 3 geo_D = 192, "
                    "M a multiple of geo_h * geo_w, a pair C and no R");
        mlp2_x3_kernel<12, 2, true, true><<<grid, 64 * MW, 0, s>>>(a);
        return cmt_check_launch("cmt_mlp2_x3");
    }
    switch (a.K / 16) {
#define MLP_K(KS) case KS: mlp2_x3_kernel<KS><<<grid, 64 * MW, 0, s>>>(a); break;
        MLP_K(1) MLP_K(2) MLP_K(3) MLP_K(4) MLP_K(5) MLP_K(6) MLP_K(7) MLP_K(8) MLP_K(9) MLP_K(10) MLP_K(11)
        MLP_K(12)
#undef MLP_K
        default: return cmt_fail(CMT_ENOTSUP, "cmt_mlp2_x3: unsupported K");
    }
    return cmt_check_launch("cmt_mlp2_x3");
}
