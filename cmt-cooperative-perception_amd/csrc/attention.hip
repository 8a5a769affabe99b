// Multi-head attention forward, head_dim = 32, for gfx950 (flash-style).
//
// Five kernel families, chosen by attn_fwd_impl (see 'Path choice'):
//   attn_pb2_kernel      f16 / bf16, long key ranges: 8 waves, ping-pong schedule
//   attn_kw_kernel       f16 / bf16, <= 64 key tiles: KW waves split the keys of 32 queries
//   attn_kw_pair_kernel  split-f16 (CMT_F16P), the same workgroup structure
//   attn_fwd_kernel      f16 / bf16, anything else: 4 waves, split partials
//   attn_fwd_f32_kernel  exact f32
// and attn_combine_kernel for the split partials.  The pieces they share are
// defined once, below AttnKParams: head_ctx (workgroup prologue), load_qf
// (Q^T fragments), acc_key / mask_keys (accumulator register -> key, ragged
// tile), vt_frag (V^T fragment), write_row (a finished query row).  Code
// generation here is sensitive to where a helper is called from: a helper
// called from another __forceinline__ function leaves the caller's code as it
// was, one called from a kernel body does not.  attn_pb2_kernel and
// attn_kw_pair_kernel are held to their former instruction streams, so their
// bodies keep the prologue and the write written out (the pair kernel also its
// mask loop), and the two KW kernels keep their ring loop and merge for the
// same reason.  attn_fwd_f32_kernel writes its mask loop out as well: through
// mask_keys it needs 160 VGPRs instead of 152.
//
// attn_fwd_kernel: one workgroup = 4 waves = 128 query rows of one (batch,
// head) and one slice of the key range ("kv split").  Each wave owns 32
// queries.  Keys are consumed in 64-key tiles staged through an LDS ring (K and
// V, 4 KB each); the next tiles' LDS-DMA is in flight while the current tile
// is computed.
//
// Per 64-key tile and wave (swapped-QK^T form, MI355X guide T12 / 'An
// accumulator tile as the next MFMA's operand'):
//   S^T[key][q] = K . Q^T      4 x v_mfma_f32_32x32x16   (K rows by ds_read_b128,
//                                                         XOR-swizzled LDS image)
//   online softmax per query   lane = query, 32 of the 64 scores per lane,
//                              partner lane (l ^ 32) holds the other 32
//   O^T[d][q] += V^T . P^T     4 x v_mfma_f32_32x32x16   (P^T straight from the
//                              S^T accumulators, V^T by ds_read_b64_tr_b16)
// With kv_splits > 1 each split writes unnormalised partial O with its running
// max / row-sum and a combine kernel merges them (flash-decoding style), so a
// 900-query problem still fills 256 CUs.
#include "cmt_common.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace {

constexpr int KT = 64;     // keys per tile
// Deferred rescale (guide T13): the running max is only raised when a score
// exceeds it by more than this many exp2 units, so P <= 2^8 (safe for f16 P)
// and the O / row-sum rescale runs on a few tiles instead of whenever any
// lane's max grows.  O = sum(P V) / sum(P) is invariant to the offset; only
// the magnitude at which P is rounded to f16/bf16 changes (same relative
// precision).
constexpr float kDeferMax = 8.f;
constexpr int QW = 32;     // queries per wave
constexpr int NW = 4;      // waves per workgroup (attn_fwd_kernel, attn_fwd_f32_kernel)
constexpr int QB = QW * NW;
constexpr int D = 32;

// Bounded-max mode (bf16 P only): exp2 units below which the Cauchy-Schwarz
// bound |q| * max|k| may serve as the fixed softmax offset of a query row
// (s - bound >= -2 * bound >= -2 * kBoundMax stays a normal bf16/f32 number).
constexpr float kBoundMax = 60.f;

struct AttnKParams {
    int B, H, Nq, Nk;
    int nqb;                        // query blocks per (b, h) (ping-pong kernel's 1-D grid)
    const float* kmax2;             // optional: per-row-block max |k|^2 partials [e][kmax_ld]
    int kmax_ld, kmax_plane0, kmax_rows;
    const void* Q; int64_t q_bs, q_hs, q_rs;
    const void* K; int64_t k_bs, k_hs, k_rs;
    const void* V; int64_t v_bs, v_hs, v_rs;
    void* O; int64_t o_bs, o_rs;    // splits == 1: final output (o_dtype)
    int o_dtype;
    float* Op; float* Mp; float* Lp; // splits > 1: partials [split][b][h][q]
    float c;                        // scale * log2(e)
    int splits;
    int tiles_per_split;
    int round_out;                  // 0, or the dtype code to round O to (CMT_ATTN_ROUND_OUTPUT)
    float* lse;                     // optional (training forward, attn_pb2_kernel path): per (b, h, q)
                                    // row statistic log2(sum exp2(s)) in exp2 units, [b][h][q]
};

// Final normalised output: 4 consecutive head dims of one query row.  A
// CMT_F16P row holds the H*32 hi values, then the H*32 lo values.
__device__ __forceinline__ void store_o4(const AttnKParams& p, int b, int q, int d0, f32x4 v) {
    const int64_t idx = (int64_t)b * p.o_bs + (int64_t)q * p.o_rs + d0;
    if (p.o_dtype == CMT_F16P) {
        store_pair4((pair_t*)p.O + idx - d0, p.H * D, d0, v);
    } else if (p.o_dtype == CMT_F32) {
        *(f32x4*)((float*)p.O + idx) = v;
    } else if (p.o_dtype == CMT_F16) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        *(h4*)((f16_t*)p.O + idx) = h4{(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]};
    } else {
        typedef __bf16 b4 __attribute__((ext_vector_type(4)));
        *(b4*)((bf16_t*)p.O + idx) = b4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    }
}

// ---- pieces every kernel family shares --------------------------------------
// A workgroup's (batch, head), its Q / K / V planes, and this lane's query row
// clamped into [0, Nq) (padding lanes of the last query block compute a copy of
// the last row and write nothing).
template <typename T>
struct HeadCtx {
    int b, h;
    const T *Q, *K, *V;
    int qc;
};
template <typename T>
__device__ __forceinline__ HeadCtx<T> head_ctx(const AttnKParams& p, int bh, int q) {
    HeadCtx<T> x;
    x.b = bh / p.H;
    x.h = bh - x.b * p.H;
    x.Q = (const T*)p.Q + (int64_t)x.b * p.q_bs + (int64_t)x.h * p.q_hs;
    x.K = (const T*)p.K + (int64_t)x.b * p.k_bs + (int64_t)x.h * p.k_hs;
    x.V = (const T*)p.V + (int64_t)x.b * p.v_bs + (int64_t)x.h * p.v_hs;
    x.qc = q < p.Nq ? q : p.Nq - 1;
    return x;
}

// The two Q^T fragments of one query row (B operand of S^T = K Q^T):
// B[k = 8*lh + j][col = q] = Q[q][16*ks + 8*lh + j].  FOLD: times c, rounded to T.
template <typename T, bool FOLD>
__device__ __forceinline__ void load_qf(const T* qrow, int lh, float c, typename mfma_traits<T>::frag (&qf)[2]) {
    typedef typename mfma_traits<T>::frag frag;
    qf[0] = *(const frag*)(qrow + 8 * lh);
    qf[1] = *(const frag*)(qrow + 16 + 8 * lh);
    if (FOLD) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[i][j] = (T)((float)qf[i][j] * c);
    }
}

// Register r of a 32x32 accumulator tile in lane half lh holds row (here: key)
// key0 + acc_key: 4 consecutive rows per 8, the halves 4 apart.
__device__ __forceinline__ int acc_key(int key0, int r, int lh) { return key0 + (r & 3) + 8 * (r >> 2) + 4 * lh; }

// Ragged last tile: the scores of keys >= Nk become -inf (key0 = key of s's row 0).
__device__ __forceinline__ f32x16 mask_keys(f32x16 s, int key0, int Nk, int lh) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (acc_key(key0, r, lh) >= Nk) s[r] = -__builtin_inff();
    return s;
}

// A V^T fragment (A operand of O^T += V^T P^T) by two transposed LDS reads
// (ds_read_b64_tr_b16) 8 key rows apart: lane 4q+p of each 16-lane group
// addresses row (r0 + q), columns dgrp + 4p .. +3; a = that byte address.
template <typename F>
__device__ __forceinline__ F vt_frag(const char* a, int rows8) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((CMT_LDS s16v4_lds*)a);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((CMT_LDS s16v4_lds*)(a + rows8));
    s16x8 vv;
    vv[0] = lo[0]; vv[1] = lo[1]; vv[2] = lo[2]; vv[3] = lo[3];
    vv[4] = hi[0]; vv[5] = hi[1]; vv[6] = hi[2]; vv[7] = hi[3];
    return __builtin_bit_cast(F, vv);
}

// A finished query row (lane = query, half lh: head dims 8g + 4lh .. +3 in
// o[4g .. 4g+3]): splits == 1 writes O / l_tot, rounded to R first when
// round_out is set (flash-attn returns the input dtype; R = float: never);
// otherwise the split's unnormalised partial with its row sum and the offset
// m2 (exp2 units) its P was taken against, for attn_combine_kernel.
template <typename R>
__device__ __forceinline__ void write_row(const AttnKParams& p, int b, int h, int split, int q, int lh,
                                          const f32x16& o, float l_tot, float m2) {
    if (p.splits == 1) {
        const float inv = 1.f / l_tot;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
            if constexpr (!std::is_same<R, float>::value) {
                if (p.round_out) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (float)(R)v[j];
                }
            }
            store_o4(p, b, q, h * D + 8 * g + 4 * lh, v);
        }
    } else {
        const int64_t row = (((int64_t)split * p.B + b) * p.H + h) * p.Nq + q;
        float* dst = p.Op + row * D;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
            *(f32x4*)(dst + 8 * g + 4 * lh) = v;
        }
        if (lh == 0) {
            p.Mp[row] = m2;
            p.Lp[row] = l_tot;
        }
    }
}

// One 64-key tile for one wave: S^T = K Q^T, online softmax, O^T += V^T P^T.
// MASK = keys >= Nk in this tile are set to -inf (only the ragged last tile).
// The running maximum enters the QK^T chain as its accumulator input (negm =
// -m_run, kept in registers across tiles), so the MFMA returns s' = s - m and
// no accumulator is zero-filled per tile.  FOLD = Q was pre-multiplied by
// c = scale*log2(e) (s' is then already in exp2 units); otherwise the
// exponent is exp2(c * s').  Scores above the running max shift m (always on
// a split's first tile, where m_run = 0 is a placeholder); the shift
// rescales O and the row sums (exact lazy rescale, rare after the first tiles).
// Row sums in fp32 of the unrounded exponentials, as flash-attn 0.2.2 sums them
// (before P is packed to the compute dtype): lsum[0] holds the lane's partial
// over its half of the tile's keys; pair_sum gives the query's total.
template <typename T, bool MASK, bool FOLD>
__device__ __forceinline__ void attn_tile_lowp(const T* __restrict__ Kt, const T* __restrict__ Vt,
                                               const typename mfma_traits<T>::frag (&qf)[2], f32x16& o,
                                               f32x16& lsum, f32x16& negm, float& m_run, bool first, float c,
                                               int key0, int Nk, int lane) {
    typedef typename mfma_traits<T>::frag frag;
    const float u = FOLD ? 1.f : c;   // s' units -> exp2 units
    const int lr = lane & 31;
    const int lh = lane >> 5;
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int row = kb * 32 + lr;
        const frag k0 = *(const frag*)(&Kt[row * D + 8 * ((lh) ^ ((row >> 2) & 3))]);
        const frag k1 = *(const frag*)(&Kt[row * D + 8 * ((2 + lh) ^ ((row >> 2) & 3))]);
        s[kb] = mfma_traits<T>::mma(k0, qf[0], negm);
        s[kb] = mfma_traits<T>::mma(k1, qf[1], s[kb]);
    }
    if (MASK) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) s[kb] = mask_keys(s[kb], key0 + kb * 32, Nk, lh);
    }
    // tile max (two v_max3 chains), then across the lane pair holding the same query
    float m0 = vmax(s[0][0], s[0][1]), m1 = vmax(s[1][0], s[1][1]);
#pragma unroll
    for (int r = 2; r < 16; r += 2) {
        m0 = vmax3(m0, s[0][r], s[0][r + 1]);
        m1 = vmax3(m1, s[1][r], s[1][r + 1]);
    }
    const float mt = pair_max(vmax(m0, m1));
    if (first || __any(mt > (FOLD ? kDeferMax : kDeferMax / c))) {
        const float d = first ? mt : vmax(mt, 0.f);
        // first tile: O and the sums are still 0 and -d may be huge (exp2 overflow -> 0*inf)
        const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-d * u);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[r] *= alpha;
            lsum[r] *= alpha;
            s[0][r] -= d;
            s[1][r] -= d;
        }
        m_run += d;
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = -m_run;
    }
    frag pf[2][2];
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float e0 = __builtin_amdgcn_exp2f(FOLD ? s[0][r] : s[0][r] * u);
        const float e1 = __builtin_amdgcn_exp2f(FOLD ? s[1][r] : s[1][r] * u);
        ps += e0 + e1;
        pf[0][r >> 3][r & 7] = (T)e0;
        pf[1][r >> 3][r & 7] = (T)e1;
    }
    lsum[0] += ps;
    const int dgrp = 16 * ((lane >> 4) & 1);
    const int tq = (lane & 15) >> 2;
    const int tp = lane & 3;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const int r0 = kb * 32 + 16 * ss + 4 * lh + tq;
            const frag vf = vt_frag<frag>((const char*)&Vt[r0 * D + dgrp + 4 * tp], 8 * D * (int)sizeof(T));
            o = mfma_traits<T>::mma(vf, pf[kb][ss], o);
        }
}

// K/V tiles arrive by LDS-DMA (global_load_lds_dwordx4) into a ring of
// RING stages, RING-1 tiles ahead of the compute, with counted vmcnt waits and
// one barrier per tile: a wave-instruction copies 16 key rows (1 KB) of K or V;
// the K image's 16-byte chunk swizzle is applied to the source address.
constexpr int RING = 4;

// One 16-byte-per-lane LDS-DMA piece (global_load_lds_dwordx4, 1 KB per wave)
// issued from inline asm.  Issued through the builtin, the compiler's waitcnt
// pass treats every later ds_read as a possible reader of the DMA'd bytes and
// puts an s_waitcnt vmcnt(0) in front of it (observed before the transposed V
// reads: it drained the whole K/V prefetch ring every tile).  As asm the DMA
// is invisible to that pass; the kernels order it themselves with counted
// vmcnt waits + barriers (which over-wait, never under-wait, for the
// compiler's own loads: in-order completion).
__device__ __forceinline__ void dma16(const void* g, const void* lds_base) {
    const uint32_t m = (uint32_t)(uintptr_t)(laddr_t)lds_base;
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(m) : "memory", "m0");
}

template <typename T, bool FOLD>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel(AttnKParams p) {
    typedef typename mfma_traits<T>::frag frag;
    constexpr int PERT = 8 / NW;                   // glds per thread per tile (8 KB / (NW KB))
    constexpr int STAGE = 2 * KT * D;              // elements: K tile then V tile
    __shared__ __attribute__((aligned(16))) T ring[RING * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;
    const int lh = lane >> 5;
    const int split = blockIdx.z;
    const int q = blockIdx.x * QB + wave * QW + lr;
    const HeadCtx<T> hc = head_ctx<T>(p, blockIdx.y, q);
    const float c = p.c;
    frag qf[2];
    load_qf<T, FOLD>(hc.Q + (int64_t)hc.qc * p.q_rs, lh, c, qf);

    const int ntiles = (p.Nk + KT - 1) / KT;
    const int t_begin = split * p.tiles_per_split;
    const int t_end = min(ntiles, t_begin + p.tiles_per_split);
    const int nt = t_end - t_begin;
    const bool ragged = (p.Nk % KT) != 0;

    // this thread's copies: id = i*NW + wave -> (K|V, 16-row block); lane -> (row, chunk)
    const int crow = lane >> 2, cch = lane & 3;
    auto issue = [&](int slot, int t) {
        T* st = ring + slot * STAGE;
#pragma unroll
        for (int i = 0; i < PERT; ++i) {
            const int id = i * NW + wave;
            const int kv = id >> 2;
            const int row = (id & 3) * 16 + crow;
            const int key = min(t * KT + row, p.Nk - 1);       // ragged tail: clamped, masked in compute
            const T* src = kv == 0 ? hc.K + (int64_t)key * p.k_rs + 8 * (cch ^ ((row >> 2) & 3))
                                   : hc.V + (int64_t)key * p.v_rs + 8 * cch;
            glds16(src, st + kv * KT * D + (id & 3) * 16 * D);
        }
    };

    f32x16 o, lsum, negm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o[r] = 0.f;
        lsum[r] = 0.f;
        negm[r] = 0.f;
    }
    float m_run = 0.f;   // placeholder until the first tile sets it

#pragma unroll
    for (int i = 0; i < RING - 1; ++i)
        if (i < nt) issue(i, t_begin + i);
    for (int i = 0; i < nt; ++i) {
        const int issued = min(nt, RING - 1 + i);
        const int inflight = issued - i - 1;  // tiles allowed to stay in flight
        if (inflight >= 2) wait_vm_lgkm<2 * PERT>();
        else if (inflight == 1) wait_vm_lgkm<PERT>();
        else wait_vm_lgkm<0>();
        barrier_mem();
        // every wave is past tile i-1: its slot takes tile i + RING - 1
        if (i + RING - 1 < nt) issue((i + RING - 1) % RING, t_begin + i + RING - 1);
        const T* Kt = ring + (i % RING) * STAGE;
        const T* Vt = Kt + KT * D;
        const int t = t_begin + i;
        const bool last_ragged = ragged && t == ntiles - 1;
        if (last_ragged)
            attn_tile_lowp<T, true, FOLD>(Kt, Vt, qf, o, lsum, negm, m_run, i == 0, c, t * KT, p.Nk, lane);
        else
            attn_tile_lowp<T, false, FOLD>(Kt, Vt, qf, o, lsum, negm, m_run, i == 0, c, t * KT, p.Nk, lane);
    }

    const float l_tot = pair_sum(lsum[0]);
    if (q >= p.Nq) return;
    write_row<T>(p, hc.b, hc.h, split, q, lh, o, l_tot, FOLD ? m_run : m_run * c);
}

// ---------------------------------------------------------------------------
// Short key ranges (the decoder's self-attention, Nk = Nq = 900): one
// workgroup = KW waves on the SAME 32 queries of one (batch, head); wave w
// takes key tiles w, w + KW, ... through a private two-slot LDS ring (LDS-DMA,
// 8 pieces per tile, counted waits, no workgroup barrier in the loop), and the
// KW partial (O, row sum, offset) triples merge through LDS at the end.  No
// split partials in HBM and no combine launch: a 900 x 900 problem is 29 x H
// workgroups of KW waves, each wave ~ntiles / KW tiles deep.
//
// f16 with the scale unfolded (the 'ref' policy's cross-attention core on short
// key ranges): a pre-pass over K finds each query's exact row maximum first, so
// P = exp(s * scale - max) is rounded to f16 at the scale the reference's flash
// core rounds it (flash-attn 0.2.2 keeps one running maximum per 128-key block, so
// for the short ranges this path takes the maximum is the global one at each
// rounding; the oracle's flash_core_fp16 does the same) instead of at an online
// offset that lags it.  Costs the QK^T MFMAs once more; the path is off the
// long-key hot loop.
// ---------------------------------------------------------------------------
constexpr int KWR = 2;      // ring slots per wave
constexpr int KWO = 36;     // merge image row stride (floats): 16-byte aligned rows

template <typename T, bool FOLD, int KW>
__global__ __launch_bounds__(KW * 64) void attn_kw_kernel(AttnKParams p) {
    typedef typename mfma_traits<T>::frag frag;
    constexpr int STAGE = 2 * KT * D;   // elements: K tile then V tile
    __shared__ __attribute__((aligned(16))) T ring[KW * KWR * STAGE];
    constexpr bool EXACT = std::is_same<T, f16_t>::value && !FOLD;
    __shared__ float xm[KW][QW], xl[KW][QW], xg[EXACT ? KW : 1][QW];
    static_assert(KWR * STAGE * (int)sizeof(T) >= QW * KWO * (int)sizeof(float), "merge image fits a wave's ring");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int lh = lane >> 5;
    const int q = blockIdx.x * QW + lr;
    const HeadCtx<T> hc = head_ctx<T>(p, blockIdx.y, q);
    const float c = p.c;

    const int ntiles = (p.Nk + KT - 1) / KT;
    const int my_n = wave < ntiles ? (ntiles - 1 - wave) / KW + 1 : 0;   // tiles wave, wave + KW, ...
    const bool ragged = (p.Nk % KT) != 0;
    T* const myring = ring + wave * KWR * STAGE;

    const int crow = lane >> 2, cch = lane & 3;
    auto issue = [&](int slot, int t) {   // the whole 64-key tile t by this wave: 4 K + 4 V pieces
        T* st = myring + slot * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = i * 16 + crow;
            const int key = min(t * KT + row, p.Nk - 1);   // ragged tail: clamped, masked in compute
            dma16(hc.K + (int64_t)key * p.k_rs + 8 * (cch ^ ((row >> 2) & 3)), st + i * 16 * D);
            dma16(hc.V + (int64_t)key * p.v_rs + 8 * cch, st + KT * D + i * 16 * D);
        }
    };
    if (my_n > 0) issue(0, wave);
    if (my_n > 1) issue(1, wave + KW);

    frag qf[2];
    load_qf<T, FOLD>(hc.Q + (int64_t)hc.qc * p.q_rs, lh, c, qf);

    f32x16 o, lsum, negm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o[r] = 0.f;
        lsum[r] = 0.f;
        negm[r] = 0.f;
    }
    float m_run = 0.f;
    if constexpr (EXACT) {
        // pre-pass: this wave's row maximum over its tiles, K fragments straight from global
        // memory (row kb * 32 + lr of the tile, columns 8 lh.. and 16 + 8 lh..), then the
        // maximum over the KW waves through LDS
        float mw = -__builtin_inff();
        for (int i = 0; i < my_n; ++i) {
            const int t = wave + i * KW;
            f32x16 s[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int key = min(t * KT + kb * 32 + lr, p.Nk - 1);
                const frag k0 = *(const frag*)(hc.K + (int64_t)key * p.k_rs + 8 * lh);
                const frag k1 = *(const frag*)(hc.K + (int64_t)key * p.k_rs + 16 + 8 * lh);
                f32x16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                s[kb] = mfma_traits<T>::mma(k0, qf[0], z);
                s[kb] = mfma_traits<T>::mma(k1, qf[1], s[kb]);
            }
            if (ragged && t == ntiles - 1) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) s[kb] = mask_keys(s[kb], t * KT + kb * 32, p.Nk, lh);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) mw = vmax3(mw, s[0][r], s[1][r]);
        }
        mw = pair_max(mw);
        if (lh == 0) xg[wave][lr] = mw;
        barrier_mem();
        float M = xg[0][lr];
#pragma unroll
        for (int w = 1; w < KW; ++w) M = vmax(M, xg[w][lr]);
        m_run = M;   // finite: every query sees >= 1 key in the workgroup
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = -M;
    }
    for (int i = 0; i < my_n; ++i) {
        // tile i landed (the Q loads above are older: in-order completion covers them)
        if (i + 1 < my_n) wait_vm_lgkm<8>();
        else wait_vm_lgkm<0>();
        const T* Kt = myring + (i & 1) * STAGE;
        const T* Vt = Kt + KT * D;
        const int t = wave + i * KW;
        const bool first = !EXACT && i == 0;   // EXACT: the offset is the final maximum from the start
        if (ragged && t == ntiles - 1)
            attn_tile_lowp<T, true, FOLD>(Kt, Vt, qf, o, lsum, negm, m_run, first, c, t * KT, p.Nk, lane);
        else
            attn_tile_lowp<T, false, FOLD>(Kt, Vt, qf, o, lsum, negm, m_run, first, c, t * KT, p.Nk, lane);
        if (i + 2 < my_n) {
            wait_vm_lgkm<0>();   // the slot's ds_reads are done (lgkmcnt) before the DMA overwrites it
            issue(i & 1, wave + (i + 2) * KW);
        }
    }

    // ---- merge the KW partials through LDS (each wave's own ring region holds its O^T image)
    wait_vm_lgkm<0>();
    float* xo = (float*)myring;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = {o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
        *(f32x4*)(xo + lr * KWO + 8 * g + 4 * lh) = v;
    }
    const float l_w = pair_sum(lsum[0]);
    if (lh == 0) {
        xm[wave][lr] = my_n > 0 ? (FOLD ? m_run : m_run * c) : -__builtin_inff();   // exp2 units
        xl[wave][lr] = l_w;
    }
    barrier_mem();
    if (tid < QW * 8) {
        const int mq = tid >> 3, d0 = 4 * (tid & 7);
        const int qo = blockIdx.x * QW + mq;
        if (qo < p.Nq) {
            float M = xm[0][mq];
#pragma unroll
            for (int w = 1; w < KW; ++w) M = vmax(M, xm[w][mq]);
            float L = 0.f;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < KW; ++w) {
                const float sc = __builtin_amdgcn_exp2f(xm[w][mq] - M);   // -inf -> 0 (waves without tiles)
                L += xl[w][mq] * sc;
                const f32x4 v = *(const f32x4*)((const float*)(ring + w * KWR * STAGE) + mq * KWO + d0);
                acc += v * sc;
            }
            const float inv = 1.f / L;
            f32x4 v = acc * inv;
            if (p.round_out) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (float)(T)v[j];
            }
            store_o4(p, hc.b, qo, hc.h * D + d0, v);
        }
    }
}

// ---------------------------------------------------------------------------
// Split-f16 self-attention (dtype CMT_F16P: the 'ref' policy's fp32-accurate
// nn.MultiheadAttention core).  Q / K / V rows are f16 pairs in the head-split
// layout cmt_gemm writes for a pair C: 64 16-bit elements per (head, row) --
// the 32 hi values, then the 32 lo values.  The workgroup structure is
// attn_kw_kernel's (KW waves on the same 32 queries, wave w takes key tiles
// w, w + KW, ... through a private two-slot LDS-DMA ring, partials merged
// through LDS), with 32-key tiles (a pair tile is twice a 16-bit tile's bytes).
// Every product is three f16 MFMAs on the pairs -- hi*hi + lo*hi + hi*lo,
// ~2^-21 relative -- with fp32 accumulation:
//   S^T = K Q^T with Q * scale * log2(e) re-split in the prologue (the
//         reference scales q before its matmul, torch MultiheadAttention)
//   P = exp2(S - m) in fp32 (online max, deferred rescale), split into a pair
//   O^T += V^T P^T (pair V^T by transposed LDS reads of both halves)
// Row sums in fp32 on the VALU.
// ---------------------------------------------------------------------------
constexpr int KTP = 32;     // keys per pair tile
constexpr int PRW = 64;     // 16-bit elements per pair row (hi 32 | lo 32)

__device__ __forceinline__ void split8(const f32x4 (&x)[2], f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = x[j >> 2][j & 3];
        hi[j] = (f16_t)v;
        lo[j] = (f16_t)(v - (float)hi[j]);
    }
}

template <bool MASK>
__device__ __forceinline__ void attn_tile_pair(const f16_t* __restrict__ Kt, const f16_t* __restrict__ Vt,
                                               const f16x8 (&qh)[2], const f16x8 (&ql)[2], f32x16& o, float& l_run,
                                               f32x16& negm, float& m_run, bool first, int key0, int Nk, int lane) {
    const int lr = lane & 31;
    const int lh = lane >> 5;
    // K rows: 128 B, 16-byte chunks XOR-swizzled by row & 7 (chunks 0-3 hi, 4-7 lo)
    const int sw = lr & 7;
    const f16_t* kr = Kt + lr * PRW;
    const f16x8 kh0 = *(const f16x8*)(kr + 8 * ((lh) ^ sw));
    const f16x8 kh1 = *(const f16x8*)(kr + 8 * ((2 + lh) ^ sw));
    const f16x8 kl0 = *(const f16x8*)(kr + 8 * ((4 + lh) ^ sw));
    const f16x8 kl1 = *(const f16x8*)(kr + 8 * ((6 + lh) ^ sw));
    f32x16 s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl0, qh[0], negm, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh0, ql[0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl1, qh[1], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh1, ql[1], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh0, qh[0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh1, qh[1], s, 0, 0, 0);
    if (MASK) {   // mask_keys written out: through the helper this kernel's code changes
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (acc_key(key0, r, lh) >= Nk) s[r] = -__builtin_inff();
    }
    float mt = vmax(s[0], s[1]);
#pragma unroll
    for (int r = 2; r < 16; r += 2) mt = vmax3(mt, s[r], s[r + 1]);
    mt = pair_max(mt);
    if (first || __any(mt > kDeferMax)) {
        const float d = first ? mt : vmax(mt, 0.f);
        const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-d);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[r] *= alpha;
            s[r] -= d;
        }
        l_run *= alpha;
        m_run += d;
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = -m_run;
    }
    f16x8 ph[2], pl[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(s[r]);
        l_run += pv;
        const f16_t h = (f16_t)pv;
        ph[r >> 3][r & 7] = h;
        pl[r >> 3][r & 7] = (f16_t)(pv - (float)h);
    }
    // V^T fragments (vt_frag, attn_tile_lowp's key order), both halves
    const int dgrp = 16 * ((lane >> 4) & 1);
    const int tq = (lane & 15) >> 2;
    const int tp = lane & 3;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
        const int r0 = 16 * ss + 4 * lh + tq;
        f16x8 vf[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            vf[half] = vt_frag<f16x8>((const char*)&Vt[r0 * PRW + 32 * half + dgrp + 4 * tp], 8 * PRW * 2);
        }
        o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[1], ph[ss], o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0], pl[ss], o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0], ph[ss], o, 0, 0, 0);
    }
}

template <int KW>
__global__ __launch_bounds__(KW * 64) void attn_kw_pair_kernel(AttnKParams p) {
    constexpr int STAGE = 2 * KTP * PRW;   // 16-bit elements: K tile then V tile (8 KB)
    __shared__ __attribute__((aligned(16))) f16_t ring[KW * KWR * STAGE];
    __shared__ float xm[KW][QW], xl[KW][QW];
    static_assert(KWR * STAGE * 2 >=QW * KWO * (int)sizeof(float), "merge image fits a wave's ring");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int lh = lane >> 5;
    const int bh = blockIdx.y;
    const int b = bh / p.H;
    const int h = bh - b * p.H;

    const f16_t* Qb = (const f16_t*)p.Q + (int64_t)b * p.q_bs + (int64_t)h * p.q_hs;
    const f16_t* Kb = (const f16_t*)p.K + (int64_t)b * p.k_bs + (int64_t)h * p.k_hs;
    const f16_t* Vb = (const f16_t*)p.V + (int64_t)b * p.v_bs + (int64_t)h * p.v_hs;

    const int ntiles = (p.Nk + KTP - 1) / KTP;
    const int my_n = wave < ntiles ? (ntiles - 1 - wave) / KW + 1 : 0;
    const bool ragged = (p.Nk % KTP) != 0;
    f16_t* const myring = ring + wave * KWR * STAGE;

    // one 1 KB piece = 8 rows of 128 B; lane -> (row lane / 8, chunk lane & 7)
    const int crow = lane >> 3, cch = lane & 7;
    auto issue = [&](int slot, int t) {   // the whole 32-key tile t: 4 K + 4 V pieces
        f16_t* st = myring + slot * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = i * 8 + crow;
            const int key = min(t * KTP + row, p.Nk - 1);   // ragged tail: clamped, masked in compute
            dma16(Kb + (int64_t)key * p.k_rs + 8 * (cch ^ (row & 7)), st + i * 8 * PRW);
            dma16(Vb + (int64_t)key * p.v_rs + 8 * cch, st + KTP * PRW + i * 8 * PRW);
        }
    };
    if (my_n > 0) issue(0, wave);
    if (my_n > 1) issue(1, wave + KW);

    // Q^T fragments (load_qf's layout) of both halves, q * c re-split
    const int q = blockIdx.x * QW + lr;
    const int qc = q < p.Nq ? q : p.Nq - 1;
    f16x8 qh[2], ql[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const f16x8 hi = *(const f16x8*)(Qb + (int64_t)qc * p.q_rs + 16 * ks + 8 * lh);
        const f16x8 lo = *(const f16x8*)(Qb + (int64_t)qc * p.q_rs + 32 + 16 * ks + 8 * lh);
        f32x4 x[2];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j >> 2][j & 3] = ((float)hi[j] + (float)lo[j]) * p.c;
        split8(x, qh[ks], ql[ks]);
    }

    f32x16 o, negm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o[r] = 0.f;
        negm[r] = 0.f;
    }
    float m_run = 0.f, l_run = 0.f;
    for (int i = 0; i < my_n; ++i) {
        if (i + 1 < my_n) wait_vm_lgkm<8>();
        else wait_vm_lgkm<0>();
        const f16_t* Kt = myring + (i & 1) * STAGE;
        const f16_t* Vt = Kt + KTP * PRW;
        const int t = wave + i * KW;
        if (ragged && t == ntiles - 1)
            attn_tile_pair<true>(Kt, Vt, qh, ql, o, l_run, negm, m_run, i == 0, t * KTP, p.Nk, lane);
        else
            attn_tile_pair<false>(Kt, Vt, qh, ql, o, l_run, negm, m_run, i == 0, t * KTP, p.Nk, lane);
        if (i + 2 < my_n) {
            wait_vm_lgkm<0>();   // the slot's ds_reads are done before the DMA overwrites it
            issue(i & 1, wave + (i + 2) * KW);
        }
    }
    l_run = pair_sum(l_run);

    // ---- merge: attn_kw_kernel's, without the rounding (a change to one goes into the other)
    wait_vm_lgkm<0>();
    float* xo = (float*)myring;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = {o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
        *(f32x4*)(xo + lr * KWO + 8 * g + 4 * lh) = v;
    }
    if (lh == 0) {
        xm[wave][lr] = my_n > 0 ? m_run : -__builtin_inff();   // exp2 units
        xl[wave][lr] = l_run;
    }
    barrier_mem();
    if (tid < QW * 8) {
        const int mq = tid >> 3, d0 = 4 * (tid & 7);
        const int qo = blockIdx.x * QW + mq;
        if (qo < p.Nq) {
            float M = xm[0][mq];
#pragma unroll
            for (int w = 1; w < KW; ++w) M = vmax(M, xm[w][mq]);
            float L = 0.f;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < KW; ++w) {
                const float sc = __builtin_amdgcn_exp2f(xm[w][mq] - M);   // -inf -> 0 (waves without tiles)
                L += xl[w][mq] * sc;
                const f32x4 v = *(const f32x4*)((const float*)(ring + w * KWR * STAGE) + mq * KWO + d0);
                acc += v * sc;
            }
            store_o4(p, b, qo, h * D + d0, acc * (1.f / L));
        }
    }
}

// Wave-wide max of the max-|k|^2 partials (each covers kmax_rows key rows)
// over the key range of this workgroup's split of batch b, head h: the bound
// only has to hold for the keys this workgroup scores (the split combine
// merges per-split offsets).  16 independent loads per lane in flight; the
// first form reduced all Nk / kmax_rows partials of the head in every wave
// (2048 waves x 882 scattered loads at the fusion shape, ~4 us of prologue).
__device__ __forceinline__ float kmax_reduce(const AttnKParams& p, int b, int h, int split, int lane) {
    const int key0 = split * p.tiles_per_split * KT;
    const int key1 = min(p.Nk, key0 + p.tiles_per_split * KT);
    if (key0 >= key1) return 0.f;
    const int64_t r0 = (int64_t)b * p.Nk;
    const int e0 = (int)((r0 + key0) / p.kmax_rows), e1 = (int)((r0 + key1 - 1) / p.kmax_rows);
    const float* src = p.kmax2 + p.kmax_plane0 + h;
    float km = 0.f;
    for (int base = e0 + lane; base <= e1; base += 64 * 16) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = base + 64 * j;
            v[j] = e <= e1 ? src[(int64_t)e * p.kmax_ld] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) km = fmaxf(km, v[j]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) km = fmaxf(km, __shfl_xor(km, off));
    return km;
}

// ---------------------------------------------------------------------------
// Long-key kernel (the cross-attention shape: Nk >= 4096, Nq > 128), f16/bf16,
// 8 waves, two 64-key tiles per ping-pong window.
//
// Bounded offsets (with the K projection's max-|k| partials): the scores of
// query q over this split's keys are <= bound_q = |q| max|k| (Cauchy-Schwarz),
// so the softmax needs no running max:
//  * bf16: when every bound of the wave is <= kBoundMax (60 exp2 units), P =
//    exp2(s) lies in [2^-60, 2^60] -- a normal bf16 / f32 number whose
//    relative rounding does not depend on its magnitude -- and the QK^T MFMAs
//    start from zero: no max tree, no subtraction, no rescale.
//  * f16 (flash-attn 0.2.2's P precision): the offset is bound_q - 15, fed in
//    as the QK^T accumulator's initial value, so P = exp2(s - bound_q + 15)
//    <= 2^15 can never overflow f16.  A loose bound only lowers P; the row
//    total then tells whether the P of this row kept full f16 precision
//    (l >= 2^-6, kF16MinSum: the absolute f16 spacing 2^-24 is then far below
//    the result's own rounding).  A workgroup with a row below it runs its
//    split again with the online maximum for the waves concerned (the slow
//    path below) -- never taken on the decoder's data, measured by
//    test_gpu_kernels.py's loose-bound cases.
// Without partials, or a bf16 bound above kBoundMax, a wave tracks an online
// running max as ONE register per lane, subtracted on the VALU (exact lazy
// rescale, deferred by kDeferMax so P <= 2^8).
//
// Q carries the folded scale c = scale * log2(e) (s in exp2 units).  QS: q * c
// is kept as hi + lo in T (both QK^T MFMA passes), the product of the stored
// q and c to ~2^-22 -- the scores of the unfolded kernel (flash-attn computes
// q k in fp32 and scales after); without QS it is rounded once to T (the
// CMT_ATTN_FOLD_SCALE permission of the f16 / bf16 speed policies).
//
// Schedule: 8 waves = two halves of 4 (wave w on SIMD w % 4, so every SIMD
// holds one wave of each half).  A wave's work per window (tiles 2j, 2j+1) is
// a matrix segment M(j) = {QK^T of the pair j, PV + row sums of pair j-1} and
// a vector segment V(j) = {exponentials of pair j}; every segment ends at a
// workgroup barrier, and half B runs one segment behind half A, so one wave
// of each SIMD issues MFMAs while its partner issues exponentials
// (MI355X_MICROARCH.md 'Two waves per SIMD').  Half A stages the K/V tiles by
// LDS-DMA into a PB2_RING-slot ring: tiles 2j+6, 2j+7 at the start of M(j),
// into the slots of pair j-3, which half B last read in V(j-2).  A leftover
// odd tile and the ragged last tile run after the loop with every wave at
// once.  Row sums on v_mfma_f32_16x16x32 with a selector A operand: the P^T
// fragment (32x32x16 B layout: lane L = query L%32, keys 8*(L/32)..+8) read as
// a 16x16x32 B operand puts query L%32 at column L%16 in k-group L/16, so
// queries q < 16 sit in k-groups 0, 2 and q >= 16 in k-groups 1, 3; selector
// rows 0 / 1 pick them (D[0][n] = query n, D[1][n] = query n + 16).
// ---------------------------------------------------------------------------
constexpr int PB2_RING = 10;
constexpr float kF16Top = 15.f;
constexpr float kF16MinSum = 0.015625f;

__device__ __forceinline__ void pp_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// LDS -> register fragments of one tile: K rows (A operand of S^T = K Q^T,
// XOR-swizzled image) and V^T (vt_frag).
// The lane-dependent parts of the addresses are byte offsets (PpLane) that the
// caller re-launders per use (empty asm), so every read is lane base +
// compile-time immediate -- no per-slot address registers kept live.
struct PpLane {
    int k0, k1;   // K row lr, chunks (lh ^ sw) and (2 + lh) ^ sw
    int v;        // V^T transposed-read base
};

__device__ __forceinline__ PpLane pp_lane(int lane, int esz) {
    const int lr = lane & 31;
    const int lh = lane >> 5;
    const int sw = (lr >> 2) & 3;
    PpLane l;
    l.k0 = (lr * D + 8 * (lh ^ sw)) * esz;
    l.k1 = (lr * D + 8 * ((2 + lh) ^ sw)) * esz;
    l.v = ((4 * lh + ((lane & 15) >> 2)) * D + 16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * esz;
    return l;
}

__device__ __forceinline__ PpLane pp_launder(PpLane l) {
    asm volatile("" : "+v"(l.k0), "+v"(l.k1), "+v"(l.v));
    return l;
}

// Kt / Vt: tile base (compile-time offset into the ring), byte-addressed
template <typename T>
__device__ __forceinline__ void pp_load_k(const char* Kt, const PpLane& l, typename mfma_traits<T>::frag (&kf)[2][2]) {
    typedef typename mfma_traits<T>::frag frag;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        kf[kb][0] = *(const frag*)(Kt + l.k0 + kb * 32 * D * (int)sizeof(T));
        kf[kb][1] = *(const frag*)(Kt + l.k1 + kb * 32 * D * (int)sizeof(T));
    }
}

template <typename T>
__device__ __forceinline__ void pp_load_v(const char* Vt, const PpLane& l, typename mfma_traits<T>::frag (&vf)[2][2]) {
    typedef typename mfma_traits<T>::frag frag;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            vf[kb][ss] = vt_frag<frag>(Vt + l.v + (kb * 32 + 16 * ss) * D * (int)sizeof(T), 8 * D * (int)sizeof(T));
        }
}

// row-sum selector (see above) and the 16x16x32 row-sum MFMA in T
template <typename T>
__device__ __forceinline__ typename mfma_traits<T>::frag rs16_selector(int lane) {
    const int m = lane & 15, g = lane >> 4;
    const T v = (T)((m == 0 && (g & 1) == 0) || (m == 1 && (g & 1) == 1) ? 1.f : 0.f);
    typename mfma_traits<T>::frag a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = v;
    return a;
}
template <typename T>
__device__ __forceinline__ f32x4 rs16_mma(const typename mfma_traits<T>::frag& pf, f32x4 l, int lane) {
    if constexpr (std::is_same<T, bf16_t>::value)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(rs16_selector<T>(lane), pf, l, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(rs16_selector<T>(lane), pf, l, 0, 0, 0);
}
// query lr's row sum from the row-sum accumulator
__device__ __forceinline__ float rs16_total(const f32x4& l, int lane) {
    const int src = lane & 15;
    const float a0 = __shfl(l[0], src), a1 = __shfl(l[1], src);
    return (lane & 31) < 16 ? a0 : a1;
}
// online-max rescale of the row-sum accumulator (alpha is per query = per lane L%32)
__device__ __forceinline__ void rs16_scale(f32x4& l, float alpha, int lane) {
    const float hi = __shfl(alpha, (lane & 15) + 16);
    l[0] *= alpha;
    l[1] *= hi;
}

// M segment of one tile on prefetched fragments: S^T = K Q^T into s (QK;
// accumulator init sinit; QS adds the lo half of Q), then O^T += V^T P^T and
// the row sums of the previous tile's P (PV) -- MFMAs only.
template <typename T, bool QK, bool PV, bool QS>
__device__ __forceinline__ void pb_mseg(const typename mfma_traits<T>::frag (&kf)[2][2],
                                        const typename mfma_traits<T>::frag (&vf)[2][2],
                                        const typename mfma_traits<T>::frag (&qf)[2],
                                        const typename mfma_traits<T>::frag (&ql)[2], const f32x16& sinit,
                                        const typename mfma_traits<T>::frag (&pf)[2][2], f32x16 (&s)[2], f32x16& o,
                                        f32x4& lsum) {
    if (QK) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = mfma_traits<T>::mma(kf[kb][0], qf[0], sinit);
            s[kb] = mfma_traits<T>::mma(kf[kb][1], qf[1], s[kb]);
            if constexpr (QS) {
                s[kb] = mfma_traits<T>::mma(kf[kb][0], ql[0], s[kb]);
                s[kb] = mfma_traits<T>::mma(kf[kb][1], ql[1], s[kb]);
            }
        }
    }
    if (PV) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                o = mfma_traits<T>::mma(vf[kb][ss], pf[kb][ss], o);
                lsum = rs16_mma<T>(pf[kb][ss], lsum, lane_id());
            }
    }
}

// online-max step over the scores of NT tiles (slow path): raise m_run when a
// score exceeds it by more than kDeferMax (always on the first tiles), rescale
// O and the row sums, subtract m_run from the scores
template <int NTL>
__device__ __forceinline__ void pb_online(f32x16* const (&s)[NTL], f32x16& o, f32x4& lsum, float& m_run, bool first) {
    float m = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) m = vmax3(m, s[t][kb][r], s[t][kb][r + 1]);
    const float mt = pair_max(m);
    if (first) {
        m_run = mt;
    } else if (__any(mt > m_run + kDeferMax)) {
        const float mn = vmax(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - mn);
        o *= alpha;
        rs16_scale(lsum, alpha, lane_id());
        m_run = mn;
    }
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][kb][r] -= m_run;
}

// V segment of one tile: P = exp2(s) into the fragments (fast) or after the online step
template <typename T>
__device__ __forceinline__ void pb_vseg(f32x16 (&s)[2], typename mfma_traits<T>::frag (&pf)[2][2], f32x16& o,
                                        f32x4& lsum, float& m_run, bool fast, bool first) {
    if (!fast) {
        f32x16* const ss[1] = {s};
        pb_online<1>(ss, o, lsum, m_run, first);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        pf[0][r >> 3][r & 7] = (T)__builtin_amdgcn_exp2f(s[0][r]);
        pf[1][r >> 3][r & 7] = (T)__builtin_amdgcn_exp2f(s[1][r]);
    }
}

// V segment of a pair, ONE online-max update for both tiles on the slow path
template <typename T>
__device__ __forceinline__ void pb2_vseg(f32x16 (&s0)[2], f32x16 (&s1)[2], typename mfma_traits<T>::frag (&pf0)[2][2],
                                         typename mfma_traits<T>::frag (&pf1)[2][2], f32x16& o, f32x4& lsum,
                                         float& m_run, bool fast, bool first) {
    if (!fast) {
        f32x16* const ss[2] = {s0, s1};
        pb_online<2>(ss, o, lsum, m_run, first);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        pf0[0][r >> 3][r & 7] = (T)__builtin_amdgcn_exp2f(s0[0][r]);
        pf0[1][r >> 3][r & 7] = (T)__builtin_amdgcn_exp2f(s0[1][r]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        pf1[0][r >> 3][r & 7] = (T)__builtin_amdgcn_exp2f(s1[0][r]);
        pf1[1][r >> 3][r & 7] = (T)__builtin_amdgcn_exp2f(s1[1][r]);
    }
}

// tiles (two LDS-DMA pieces each) still allowed in flight behind the ones needed now, 0..4
__device__ __forceinline__ void pb2_wait(int tiles) {
    if (tiles >= 4) wait_vm_lgkm<8>();
    else if (tiles == 3) wait_vm_lgkm<6>();
    else if (tiles == 2) wait_vm_lgkm<4>();
    else if (tiles == 1) wait_vm_lgkm<2>();
    else wait_vm_lgkm<0>();
}

// US (f16, bounded offsets or not): Q enters the QK^T MFMAs unscaled, exactly the f16 q the
// reference's flash core multiplies, and the vector segment applies s * c - offset in fp32 (one
// packed FMA per two scores) -- flash-attn's own order (q k in fp32, then the scale), with half
// the QK^T MFMAs of QS.
template <typename T, bool QS, bool US = false>
__global__ __launch_bounds__(512, 2) void attn_pb2_kernel(AttnKParams p) {
    static_assert(!(QS && US), "QS and US are alternatives");
    typedef typename mfma_traits<T>::frag frag;
    constexpr bool F16 = std::is_same<T, f16_t>::value;
    constexpr int STAGE = 2 * KT * D;   // elements: K tile then V tile
    __shared__ __attribute__((aligned(16))) T ring[PB2_RING * STAGE];
    __shared__ int redo;                // f16: some row of the workgroup needs the online-max pass

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool hb = wave >= 4;          // wave-uniform: second half runs one segment behind
    const int lr = lane & 31;
    const int lh = lane >> 5;
    if (tid == 0) redo = 0;

    // XCD-aware block order: consecutive query blocks of one (b, h, split) on one XCD (shared K/V in its L2)
    const int nwg = gridDim.x;
    const int orig = blockIdx.x;
    const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    const int qb = wg % p.nqb;
    const int rest = wg / p.nqb;
    const int BH = p.B * p.H;
    const int bh = rest % BH;
    const int split = rest / BH;
    const int b = bh / p.H;
    const int h = bh - b * p.H;

    // a wave whose 32 queries all lie past Nq (the padding of the last query block) keeps the
    // workgroup's barriers and LDS-DMA duties but skips its MFMAs, exponentials and fragment reads
    const bool live = qb * (8 * QW) + wave * QW < p.Nq;
    const T* Qb = (const T*)p.Q + (int64_t)b * p.q_bs + (int64_t)h * p.q_hs;
    const T* Kb = (const T*)p.K + (int64_t)b * p.k_bs + (int64_t)h * p.k_hs;
    const T* Vb = (const T*)p.V + (int64_t)b * p.v_bs + (int64_t)h * p.v_hs;
    const float c = p.c;

    const int ntiles = (p.Nk + KT - 1) / KT;
    const int t_begin = split * p.tiles_per_split;
    const int t_end = min(ntiles, t_begin + p.tiles_per_split);
    const bool tail = (p.Nk % KT) != 0 && t_end == ntiles && t_begin < t_end;   // ragged last tile here
    const int nt = max(0, t_end - t_begin - (tail ? 1 : 0));                    // full tiles
    const int np = nt >> 1;                                                      // full tile pairs

    const int crow = lane >> 2, cch = lane & 3;
    const int prow = (wave & 3) * 16 + crow;
    const T* const ksrc0 = Kb + (int64_t)(t_begin * KT + prow) * p.k_rs + 8 * (cch ^ ((prow >> 2) & 3));
    const T* const vsrc0 = Vb + (int64_t)(t_begin * KT + prow) * p.v_rs + 8 * cch;
    const T* ksrc = ksrc0;
    const T* vsrc = vsrc0;
    const int64_t kstep = (int64_t)KT * p.k_rs, vstep = (int64_t)KT * p.v_rs;
    T* const my_k = ring + (wave & 3) * 16 * D;
    int issued = 0;   // tiles issued (half A)
    auto issue_upto = [&](int n) {   // tiles [issued, min(n, nt)) into their ring slots
        const int e = min(n, nt);
        while (issued < e) {
            T* dst = my_k + (issued % PB2_RING) * STAGE;
            dma16(ksrc, dst);
            dma16(vsrc, dst + KT * D);
            ksrc += kstep;
            vsrc += vstep;
            ++issued;
        }
    };

    const char* const rb = (const char*)ring;
    constexpr int STAGE_B = STAGE * (int)sizeof(T), KV_B = KT * D * (int)sizeof(T);
    const PpLane lane_ofs = pp_lane(lane, (int)sizeof(T));
    f32x16 s0[2], s1[2];
    frag pf0[2][2], pf1[2][2], kf0[2][2], kf1[2][2], vf0[2][2], vf1[2][2];
    // the first three pairs' LDS-DMA before the Q / max-|k| loads
    if (!hb) issue_upto(PB2_RING - 4);

    // ---- Q^T fragments with the folded scale (s is in exp2 units)
    const int q = qb * (8 * QW) + wave * QW + lr;
    const int qc = q < p.Nq ? q : p.Nq - 1;
    frag qf[2], ql[2];
    float qq = 0.f;
    {
        const frag r0 = *(const frag*)(Qb + (int64_t)qc * p.q_rs + 8 * lh);
        const frag r1 = *(const frag*)(Qb + (int64_t)qc * p.q_rs + 16 + 8 * lh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x0 = (float)r0[j] * c, x1 = (float)r1[j] * c;
            qf[0][j] = US ? r0[j] : (T)x0;
            qf[1][j] = US ? r1[j] : (T)x1;
            ql[0][j] = (T)(x0 - (float)qf[0][j]);
            ql[1][j] = (T)(x1 - (float)qf[1][j]);
            const float e0 = QS || US ? x0 : (float)qf[0][j], e1 = QS || US ? x1 : (float)qf[1][j];
            qq += e0 * e0 + e1 * e1;
        }
    }

    // ---- offset mode: bounded (fast) iff partials are given (bf16: and every bound <= kBoundMax)
    bool fast = false;
    float off = 0.f;   // f16 fast path: the fixed offset bound - kF16Top
    if (p.kmax2 != nullptr) {
        const float km = kmax_reduce(p, b, h, split, lane);
        const float bound = sqrtf(pair_sum(qq) * km) * 1.001f + 1e-6f;
        if constexpr (F16) {
            fast = true;
            off = bound - kF16Top;
        } else {
            fast = __all(bound <= kBoundMax);
        }
    }
    f32x16 sinit;
#pragma unroll
    for (int r = 0; r < 16; ++r) sinit[r] = F16 && fast && !US ? -off : 0.f;

    f32x16 o;
    f32x4 lsum;
    float m_run = 0.f;   // slow path: set by the first tiles
    // US: the raw scores q k -> exp2 units s * c - offset (fast) or s * c (online max)
    auto us_scale = [&](f32x16 (&sx)[2], bool fastw) {
        if constexpr (US) {
            const f32x2 c2 = {c, c};
            const f32x2 sub2 = fastw ? f32x2{-off, -off} : f32x2{0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2 v = __builtin_elementwise_fma(f32x2{sx[kb][r], sx[kb][r + 1]}, c2, sub2);
                    sx[kb][r] = v[0];
                    sx[kb][r + 1] = v[1];
                }
        }
    };

    // One pass over the split's keys.  fastw: bounded offsets (else online max); livew: this wave
    // computes (else it only keeps the barriers and, in half A, the LDS-DMA) and restarts O / l.
    auto run = [&](bool fastw, bool livew) {
        if (livew) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = 0.f;
            lsum = f32x4{0.f, 0.f, 0.f, 0.f};
            m_run = 0.f;
        }
        auto slot_b = [&](int t) { return rb + (t % PB2_RING) * STAGE_B; };
        if (hb) pp_barrier();   // half B: one segment behind
        if (np > 0) {
            if (!hb) pb2_wait(issued - 2);                 // tiles 0, 1 landed
            pp_barrier();
            if (!hb) issue_upto(8);
            {
                const PpLane l = pp_launder(lane_ofs);
                if (livew) pp_load_k<T>(slot_b(0), l, kf0);
                if (livew) pp_load_k<T>(slot_b(1), l, kf1);
            }
            if (livew) pb_mseg<T, true, false, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);
            if (livew) pb_mseg<T, true, false, QS>(kf1, vf1, qf, ql, sinit, pf1, s1, o, lsum);
            if (!hb && np > 1) pb2_wait(issued - 4);       // tiles 2, 3 landed
            pp_barrier();
            if (livew) us_scale(s0, fastw);
            if (livew) us_scale(s1, fastw);
            if (livew) pb2_vseg<T>(s0, s1, pf0, pf1, o, lsum, m_run, fastw, true);
            {
                const PpLane l = pp_launder(lane_ofs);
                if (livew) pp_load_k<T>(slot_b(2), l, kf0);   // stale (unused) when np == 1
                if (livew) pp_load_k<T>(slot_b(3), l, kf1);
                if (livew) pp_load_v<T>(slot_b(0) + KV_B, l, vf0);
                if (livew) pp_load_v<T>(slot_b(1) + KV_B, l, vf1);
            }
            for (int j = 1; j < np; ++j) {
                pp_barrier();
                if (!hb) issue_upto(2 * j + 8);
                if (livew) pb_mseg<T, true, true, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);   // QK^T 2j, PV 2j-2
                if (livew) pb_mseg<T, true, true, QS>(kf1, vf1, qf, ql, sinit, pf1, s1, o, lsum);   // QK^T 2j+1, PV 2j-1
                if (!hb && j + 1 < np) pb2_wait(issued - (2 * j + 4));       // tiles 2j+2, 2j+3 landed
                pp_barrier();
                if (livew) us_scale(s0, fastw);
                if (livew) us_scale(s1, fastw);
                if (livew) pb2_vseg<T>(s0, s1, pf0, pf1, o, lsum, m_run, fastw, false);
                const PpLane l = pp_launder(lane_ofs);
                if (livew) pp_load_k<T>(slot_b(2 * j + 2), l, kf0);   // stale (unused) on the last pair
                if (livew) pp_load_k<T>(slot_b(2 * j + 3), l, kf1);
                if (livew) pp_load_v<T>(slot_b(2 * j) + KV_B, l, vf0);
                if (livew) pp_load_v<T>(slot_b(2 * j + 1) + KV_B, l, vf1);
            }
            pp_barrier();
            if (livew) pb_mseg<T, false, true, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);
            if (livew) pb_mseg<T, false, true, QS>(kf1, vf1, qf, ql, sinit, pf1, s1, o, lsum);
        }
        if (!hb) pp_barrier();   // half A: the window half B spends on its last PV

        if (nt & 1) {
            // leftover full tile (odd count): every wave at once
            if (!hb) {
                issue_upto(nt);
                wait_vm_lgkm<0>();
            }
            pp_barrier();
            const PpLane l = pp_launder(lane_ofs);
            if (livew) pp_load_k<T>(slot_b(nt - 1), l, kf0);
            if (livew) pp_load_v<T>(slot_b(nt - 1) + KV_B, l, vf0);
            if (livew) pb_mseg<T, true, false, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);
            if (livew) us_scale(s0, fastw);
            if (livew) pb_vseg<T>(s0, pf0, o, lsum, m_run, fastw, np == 0);
            if (livew) pb_mseg<T, false, true, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);
        }

        if (tail) {
            // ragged last tile: masked, every wave at once
            pp_barrier();
            if (!hb) {
                const int key = min((ntiles - 1) * KT + prow, p.Nk - 1);   // clamped, masked below
                const T* ks = Kb + (int64_t)key * p.k_rs + 8 * (cch ^ ((prow >> 2) & 3));
                const T* vs = Vb + (int64_t)key * p.v_rs + 8 * cch;
                dma16(ks, my_k);
                dma16(vs, my_k + KT * D);
                wait_vm_lgkm<0>();
            }
            pp_barrier();
            const PpLane l = pp_launder(lane_ofs);
            if (livew) pp_load_k<T>(rb, l, kf0);
            if (livew) pp_load_v<T>(rb + KV_B, l, vf0);
            if (livew) pb_mseg<T, true, false, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);
            const int key0 = (ntiles - 1) * KT;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) s0[kb] = mask_keys(s0[kb], key0 + kb * 32, p.Nk, lh);
            if (livew) us_scale(s0, fastw);
            if (livew) pb_vseg<T>(s0, pf0, o, lsum, m_run, fastw, nt == 0);
            if (livew) pb_mseg<T, false, true, QS>(kf0, vf0, qf, ql, sinit, pf0, s0, o, lsum);
        }
    };
    run(fast, live);
    float l_tot = rs16_total(lsum, lane);

    if constexpr (F16) {
        // a loose bound left some row's P too small for full f16 precision: those waves run the
        // split again with the online max (every wave keeps the barriers and DMA duties)
        const bool bad = fast && live && __any(!(l_tot >= kF16MinSum));
        if (bad && lane == 0) redo = 1;
        barrier_mem();   // every wave is past its last ring read and its vote is visible
        if (redo) {
            ksrc = ksrc0;
            vsrc = vsrc0;
            issued = 0;
            if (!hb) issue_upto(PB2_RING - 4);
#pragma unroll
            for (int r = 0; r < 16; ++r) sinit[r] = 0.f;
            run(false, bad);
            if (bad) {
                fast = false;
                l_tot = rs16_total(lsum, lane);
            }
        }
    }

    // ---- write
    if (q >= p.Nq) return;
    if (p.splits == 1) {
        const float inv = 1.f / l_tot;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
            if (p.round_out) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (float)(T)v[j];
            }
            store_o4(p, b, q, h * D + 8 * g + 4 * lh, v);
        }
        if (p.lse && lh == 0) p.lse[((int64_t)b * p.H + h) * p.Nq + q] = (fast ? off : m_run) + __log2f(l_tot);
    } else {
        const int64_t row = (((int64_t)split * p.B + b) * p.H + h) * p.Nq + q;
        float* dst = p.Op + row * D;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
            *(f32x4*)(dst + 8 * g + 4 * lh) = v;
        }
        if (lh == 0) {
            p.Mp[row] = fast ? off : m_run;   // exp2 units: the offset P was taken against
            p.Lp[row] = l_tot;
        }
    }
}

// ---------------------------------------------------------------------------
// Exact-f32 variant (v_mfma_f32_32x32x2_f32): same tiling and online softmax;
// used where the reference computes attention in fp32 (nn.MultiheadAttention
// self-attention).  K image rows padded to 36 floats (conflict-free
// ds_read_b128); QK^T k index permuted as d = 16*(lane>>5) + t; P stays f32 in
// the S^T accumulators and feeds the PV MFMAs directly, V^T elements by
// ds_read_b32 (one row of 32 floats per half-wave: conflict-free).
// ---------------------------------------------------------------------------
constexpr int KP = 36;

__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(AttnKParams p) {
    __shared__ __attribute__((aligned(16))) float Ks[2][KT * KP];
    __shared__ __attribute__((aligned(16))) float Vs[2][KT * D];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;
    const int lh = lane >> 5;
    const int split = blockIdx.z;
    const int q = blockIdx.x * QB + wave * QW + lr;
    const HeadCtx<float> hc = head_ctx<float>(p, blockIdx.y, q);
    f32x4 qf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qf[i] = *(const f32x4*)(hc.Q + (int64_t)hc.qc * p.q_rs + 16 * lh + 4 * i);

    const int ntiles = (p.Nk + KT - 1) / KT;
    const int t_begin = split * p.tiles_per_split;
    const int t_end = min(ntiles, t_begin + p.tiles_per_split);

    f32x4 kreg[2], vreg[2];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx >> 3, c4 = idx & 7;
            const int key = t * KT + row;
            if (key < p.Nk) {
                kreg[i] = *(const f32x4*)(hc.K + (int64_t)key * p.k_rs + 4 * c4);
                vreg[i] = *(const f32x4*)(hc.V + (int64_t)key * p.v_rs + 4 * c4);
            } else {
                kreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                vreg[i] = kreg[i];
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx >> 3, c4 = idx & 7;
            *(f32x4*)(&Ks[buf][row * KP + 4 * c4]) = kreg[i];
            *(f32x4*)(&Vs[buf][row * D + 4 * c4]) = vreg[i];
        }
    };

    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m_run = -__builtin_inff();
    float l_run = 0.f;
    const float c = p.c;

    if (t_begin < t_end) {
        load_tile(t_begin);
        store_tile(0);
    }
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        const int cur = (t - t_begin) & 1;
        if (t + 1 < t_end) load_tile(t + 1);
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
            const float* krow = &Ks[cur][(kb * 32 + lr) * KP + 16 * lh];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 kv = *(const f32x4*)(krow + 4 * i);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[j], qf[i][j], s[kb], 0, 0, 0);
            }
        }
        if ((t + 1) * KT > p.Nk) {   // mask_keys written out (VGPRs, see the file header)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (acc_key(t * KT + kb * 32, r, lh) >= p.Nk) s[kb][r] = -__builtin_inff();
        }
        float mt = s[0][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[0][r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[1][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = exp2f((m_run - m_new) * c);
        const float mc = m_new * c;
        float ls = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = exp2f(fmaf(s[kb][r], c, -mc));
                ls += e;
                s[kb][r] = e;
            }
        l_run = l_run * alpha + ls;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = Vs[cur][acc_key(kb * 32, r, lh) * D + lr];
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(v, s[kb][r], o, 0, 0, 0);
            }
        if (t + 1 < t_end) store_tile(cur ^ 1);
        __syncthreads();
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    if (q >= p.Nq) return;
    write_row<float>(p, hc.b, hc.h, split, q, lh, o, l_tot, m_run * c);
}

// Merge the kv-split partials: 8 threads per (b, h, q), each owning 4 of the
// 32 head dims.  NS = split count (compile-time, so every partial load is
// issued before the first use; the maxima are in exp2 units).
template <int NS>
__global__ __launch_bounds__(256) void attn_combine_kernel(AttnKParams p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t rows = (int64_t)p.B * p.H * p.Nq;
    if (idx >= rows * 8) return;
    const int d4 = (int)(idx & 7) * 4;
    const int64_t bhq = idx >> 3;
    const int q = (int)(bhq % p.Nq);
    const int64_t bh = bhq / p.Nq;
    const int h = (int)(bh % p.H);
    const int b = (int)(bh / p.H);
    float ms[NS], ls[NS];
    f32x4 os[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        ms[s] = p.Mp[s * rows + bhq];
        ls[s] = p.Lp[s * rows + bhq];
        os[s] = *(const f32x4*)(p.Op + (s * rows + bhq) * D + d4);
    }
    float M = -__builtin_inff();
#pragma unroll
    for (int s = 0; s < NS; ++s) M = ls[s] > 0.f ? fmaxf(M, ms[s]) : M;   // empty splits (l == 0) excluded
    f32x4 num = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        // an empty split (no keys) has l == 0 and contributes nothing
        const float w = ls[s] > 0.f ? __builtin_amdgcn_exp2f(ms[s] - M) : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) num[j] = __builtin_fmaf(w, os[s][j], num[j]);   // explicit: chain B1's
        den = __builtin_fmaf(w, ls[s], den);                                       // combine matches bitwise
    }
    const float inv = 1.f / den;
    f32x4 r = num * inv;
    if (p.round_out == CMT_F16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (float)(f16_t)r[j];
    } else if (p.round_out == CMT_BF16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (float)(bf16_t)r[j];
    }
    store_o4(p, b, q, h * D + d4, r);
    if (p.lse && d4 == 0) p.lse[bhq] = M + __log2f(den);
}

// Path choice.  Long key ranges (the cross-attention shape) take the 8-wave
// ping-pong kernel attn_pb2_kernel; short ones with at most 64 key tiles (the
// self-attention) the in-workgroup key split attn_kw_kernel; anything else the
// 4-wave single-phase attn_fwd_kernel with split partials.  f32 always takes
// the exact-f32 kernel.
// the reference-numerics f16 core (no fold permission): the per-call CMT_ATTN_UNSCALED_Q flag ->
// unscaled Q (attn_pb2_kernel US); else Q * c as hi + lo (QS)
bool us_mode(int flags) { return (flags & CMT_ATTN_UNSCALED_Q) != 0; }

bool use_long(const cmt_attn_args& a) {
    return a.dtype != CMT_F32 && a.dtype != CMT_F16P && a.Nk >= 4096 && a.Nq > 128;
}

bool use_kw(const cmt_attn_args& a) {
    if (a.dtype == CMT_F16P) return true;   // the split-f16 kernel has only the key-split form
    if (a.dtype == CMT_F32 || a.kv_splits > 0 || use_long(a)) return false;
    return (a.Nk + KT - 1) / KT <= 64;
}

// The (dtype, fold) of a 16-bit call as types: f(T{}, std::bool_constant<FOLD>{}) picks a
// kernel family's instantiation once.
template <typename F>
void lowp_case(int dtype, bool fold, F&& f) {
    if (dtype == CMT_F16) {
        if (fold) f(f16_t{}, std::true_type{});
        else f(f16_t{}, std::false_type{});
    } else {
        if (fold) f(bf16_t{}, std::true_type{});
        else f(bf16_t{}, std::false_type{});
    }
}

int choose_splits(const cmt_attn_args& a) {
    if (a.kv_splits > 0) return a.kv_splits;
    if (use_kw(a)) return 1;
    const int ntiles = (a.Nk + KT - 1) / KT;
    const int nw = a.dtype == CMT_F32 ? NW : (use_long(a) ? 8 : 4);
    const int base = cdiv(a.Nq, nw * QW) * a.B * a.H;
    if (use_long(a)) {
        // the long-key kernel (one 8-wave workgroup per CU): the launch takes ceil(workgroups / CUs)
        // rounds, each about as long as one split's key tiles plus a fixed ~10-tile prologue and
        // tail; the fewest splits of the cheapest count win (the split partials cost a combine).
        // 900 queries over 56 400 / 32 400 keys: 8 splits (one round of 256); 1 500 queries over
        // 48 400 keys (configs[4]): 5 splits, 120 vs 142 us for the former power of two 8 -- 384
        // workgroups in 1.5 rounds (profiles/r6_experiments.txt r6v)
        const int cus = cmt_cu_count();
        int best = 1;
        int64_t best_cost = INT64_MAX;
        for (int s = 1; s <= 16; ++s) {
            if (s > 1 && ntiles / s < 8) break;
            const int64_t rounds = cdiv64((int64_t)base * s, cus);
            const int64_t cost = rounds * (cdiv(ntiles, s) + 10);
            if (cost < best_cost) {
                best_cost = cost;
                best = s;
            }
        }
        return best;
    }
    int s = 1;
    // aim for >= 2048 waves (two per SIMD) while keeping >= 8 tiles per split;
    // short key ranges split down to 2 tiles per split
    const int min_tiles = ntiles >= 64 ? 8 : 2;
    while ((int64_t)base * s * nw < 2048 && ntiles / (2 * s) >= min_tiles) s *= 2;
    return s;
}

}  // namespace

extern "C" int64_t cmt_attn_workspace_bytes(const cmt_attn_args* a) {
    if (!a) return 0;
    const int s = choose_splits(*a);
    if (s <= 1) return 0;
    const int64_t rows = (int64_t)s * a->B * a->H * a->Nq;
    return rows * (D + 2) * (int64_t)sizeof(float);
}

// the training forward (attn_train.hip) runs the long-key f16 path with the row statistic
int attn_fwd_impl(const cmt_attn_args& a, float* lse, void* stream);

extern "C" int cmt_attn_fwd(const cmt_attn_args* ap, void* stream) {
    CMT_REQUIRE(ap != nullptr, "cmt_attn_fwd: null args");
    return attn_fwd_impl(*ap, nullptr, stream);
}

extern "C" int cmt_attn_splits(const cmt_attn_args* a) {
    return a ? choose_splits(*a) : 0;
}

int cmt_attn_fwd_lse(const cmt_attn_args& a, float* lse, void* stream) {
    CMT_REQUIRE(lse != nullptr && a.dtype == CMT_F16 && use_long(a) && a.kmax2 != nullptr &&
                    !(a.flags & (CMT_ATTN_FOLD_SCALE | CMT_ATTN_KEEP_PARTIALS)),
                "cmt_attn_fwd_lse: the row statistic comes from the long-key f16 bounded path only");
    return attn_fwd_impl(a, lse, stream);
}

int attn_fwd_impl(const cmt_attn_args& a, float* lse, void* stream) {
    CMT_REQUIRE(a.B > 0 && a.H > 0 && a.Nq > 0 && a.Nk > 0, "cmt_attn_fwd: empty problem");
    CMT_REQUIRE(a.dtype == CMT_F16 || a.dtype == CMT_BF16 || a.dtype == CMT_F32 || a.dtype == CMT_F16P,
                "cmt_attn_fwd: dtype must be f32, f16, bf16 or f16 pair");
    CMT_REQUIRE(a.dtype != CMT_F16P || (a.kv_splits <= 1 && a.kmax2 == nullptr && a.q_rstride >= 64 &&
                                        a.k_rstride >= 64 && a.v_rstride >= 64 && a.Nk <= (1 << 20) &&
                                        ((uintptr_t)a.Q | (uintptr_t)a.K | (uintptr_t)a.V) % 16 == 0),
                "cmt_attn_fwd: f16-pair Q/K/V take pair rows (>= 64 16-bit elements: 32 hi, 32 lo), "
                "no kv_splits / kmax2, 16-byte aligned");
    CMT_REQUIRE(a.Q && a.K && a.V && a.O, "cmt_attn_fwd: null pointer");
    CMT_REQUIRE(a.dtype != CMT_F32 || ((a.q_rstride | a.k_rstride | a.v_rstride) % 4 == 0),
                "cmt_attn_fwd: f32 rows must be 16-byte aligned");
    CMT_REQUIRE(a.o_rstride % 4 == 0 && a.o_bstride % 4 == 0, "cmt_attn_fwd: O strides must be multiples of 4");
    CMT_REQUIRE(a.o_dtype == CMT_F32 || a.o_dtype == CMT_F16 || a.o_dtype == CMT_BF16 || a.o_dtype == CMT_F16P,
                "cmt_attn_fwd: bad o_dtype");
    CMT_REQUIRE(a.q_rstride % 8 == 0 && a.k_rstride % 8 == 0 && a.v_rstride % 8 == 0 && a.q_hstride % 8 == 0 &&
                a.k_hstride % 8 == 0 && a.v_hstride % 8 == 0 && a.q_bstride % 8 == 0 && a.k_bstride % 8 == 0 &&
                a.v_bstride % 8 == 0, "cmt_attn_fwd: Q/K/V strides must be multiples of 8 elements");
    const int splits = choose_splits(a);
    CMT_REQUIRE(splits <= 16 || splits == 24 || splits == 32 || splits == 48 || splits == 64,
                "cmt_attn_fwd: kv_splits must be <= 16, 24, 32, 48 or 64");
    const int ntiles = (a.Nk + KT - 1) / KT;
    CMT_REQUIRE(a.kmax2 == nullptr || (a.kmax_rows > 0 && a.kmax_ld > 0 && a.kmax_plane0 >= 0 &&
                                       a.kmax_plane0 + a.H <= a.kmax_ld),
                "cmt_attn_fwd: bad kmax2 partials geometry");
    AttnKParams p;
    p.B = a.B; p.H = a.H; p.Nq = a.Nq; p.Nk = a.Nk;
    p.nqb = cdiv(a.Nq, 8 * QW);
    p.kmax2 = a.kmax2;
    p.kmax_ld = a.kmax_ld; p.kmax_plane0 = a.kmax_plane0; p.kmax_rows = a.kmax_rows;
    p.Q = a.Q; p.q_bs = a.q_bstride; p.q_hs = a.q_hstride; p.q_rs = a.q_rstride;
    p.K = a.K; p.k_bs = a.k_bstride; p.k_hs = a.k_hstride; p.k_rs = a.k_rstride;
    p.V = a.V; p.v_bs = a.v_bstride; p.v_hs = a.v_hstride; p.v_rs = a.v_rstride;
    p.O = a.O; p.o_bs = a.o_bstride; p.o_rs = a.o_rstride; p.o_dtype = a.o_dtype;
    p.c = a.scale * 1.4426950408889634f;
    p.splits = splits;
    p.tiles_per_split = cdiv(ntiles, splits);
    p.round_out = (a.flags & CMT_ATTN_ROUND_OUTPUT) && a.dtype != CMT_F32 ? a.dtype : 0;
    p.lse = lse;
    p.Op = p.Mp = p.Lp = nullptr;
    if (splits > 1) {
        const int64_t need = cmt_attn_workspace_bytes(&a);
        if (a.workspace == nullptr || a.workspace_bytes < need)
            return cmt_fail(CMT_EWORKSPACE, "cmt_attn_fwd: workspace too small");
        const int64_t rows = (int64_t)splits * a.B * a.H * a.Nq;
        p.Op = (float*)a.workspace;
        p.Mp = p.Op + rows * D;
        p.Lp = p.Mp + rows;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool fold = (a.flags & CMT_ATTN_FOLD_SCALE) != 0;
    if (a.dtype == CMT_F16P) {
        attn_kw_pair_kernel<8><<<dim3(cdiv(a.Nq, QW), a.B * a.H), 512, 0, s>>>(p);
        return cmt_check_launch("cmt_attn_fwd");
    }
    if (a.dtype == CMT_F32) {
        attn_fwd_f32_kernel<<<dim3(cdiv(a.Nq, QB), a.B * a.H, splits), 256, 0, s>>>(p);
    } else if (use_kw(a)) {
        const dim3 g2(cdiv(a.Nq, QW), a.B * a.H);
        lowp_case(a.dtype, fold, [&](auto t, auto f) {
            attn_kw_kernel<decltype(t), decltype(f)::value, 8><<<g2, 512, 0, s>>>(p);
        });
    } else if (use_long(a)) {
        // the scale is folded into Q either way; without the FOLD permission q * c is kept as hi + lo
        // (QS), or, f16 with CMT_ATTN_UNSCALED_Q, Q enters unscaled (US)
        const unsigned nwg = (unsigned)p.nqb * a.B * a.H * splits;
        lowp_case(a.dtype, fold, [&](auto t, auto f) {
            typedef decltype(t) T;
            constexpr bool FOLD = decltype(f)::value;
            if (std::is_same<T, f16_t>::value && !FOLD && us_mode(a.flags))
                attn_pb2_kernel<f16_t, false, true><<<nwg, 512, 0, s>>>(p);
            else
                attn_pb2_kernel<T, !FOLD><<<nwg, 512, 0, s>>>(p);
        });
    } else {
        const dim3 grid(cdiv(a.Nq, QB), a.B * a.H, splits);
        lowp_case(a.dtype, fold, [&](auto t, auto f) {
            attn_fwd_kernel<decltype(t), decltype(f)::value><<<grid, NW * 64, 0, s>>>(p);
        });
    }
    int rc = cmt_check_launch("cmt_attn_fwd");
    if (rc || splits == 1 || (a.flags & CMT_ATTN_KEEP_PARTIALS)) return rc;   // KEEP: partials for chain B1
    const int64_t total = (int64_t)a.B * a.H * a.Nq * 8;
    const unsigned nb = (unsigned)cdiv64(total, 256);
    switch (splits) {
#define COMB(NS) case NS: attn_combine_kernel<NS><<<nb, 256, 0, s>>>(p); break;
        COMB(2) COMB(3) COMB(4) COMB(5) COMB(6) COMB(7) COMB(8) COMB(9) COMB(10) COMB(11) COMB(12) COMB(13)
        COMB(14) COMB(15) COMB(16) COMB(24) COMB(32) COMB(48) COMB(64)
#undef COMB
        default: return cmt_fail(CMT_ENOTSUP, "cmt_attn_fwd: kv_splits must be <= 16, 24, 32, 48 or 64");
    }
    return cmt_check_launch("cmt_attn_combine");
}
