// Attention forward-with-statistics and backward for the training path (head_dim 32).
// Reference: the self-attention nn.MultiheadAttention (mmcv MultiheadAttention, with the
// training-time DN mask of cmt_head.py:386-398 and attn_drop) and the FlashMHA cross-attention
// core (attention.py:46-92, flash-attn 0.2.2 fp16 core: fp16_inputs rounds q, k, v, P and O to
// fp16 as that core does).
//
// Three passes, each ONE kernel template over an arithmetic policy A and the flags MASK (the DN
// mask can hide keys) and DROP (dropout):
//   fwd_kernel  one wave per 32 queries, 4 waves per workgroup share 64-key K / V tiles in LDS,
//               swapped S^T = K Q^T so a lane owns one query, online softmax in exp2 units, key
//               range split over workgroups (train_combine_kernel) so ~1000-query problems fill the
//               chip.  Writes O and the row statistic LSE2 = m + log2(l) (exp2 units of
//               c = scale * log2 e).
//   dq_kernel   (flash-style, P recomputed from LSE2, delta = rowsum(dO * O)) one wave per 32
//               queries over a key slice: S^T, dP^T = V dO^T, dS^T = P^T (dP^T - delta),
//               dQ^T += K^T dS^T (f32 atomics into a zeroed dQ when the key range is split)
//   dkv_kernel  one wave per 32 keys over a slice of the queries: S = Q K^T, dV^T += dO^T P,
//               dP = dO V^T, dS = P (dP - delta), dK^T += Q^T dS (f32 atomics into zeroed dK / dV
//               when the queries are split)
// Every product's accumulator layout is the next product's B operand (lane = the free index,
// registers = the contraction index), so no tile is transposed through LDS.
//
// The policy supplies what differs between the arithmetics: how a 64-row tile is staged in LDS
// (TILE bytes, stage), a lane's own row in registers (Own, load_own), "32 tile rows x own row"
// (rows_x_own: S, dP), "tile rows^T x fp32 accumulator tile" (tr_x_acc: O, dQ, dK, dV), how O is
// rounded and which exp2 the softmax uses.
//   F32  exact f32 on v_mfma_f32_32x32x2_f32, padded float rows
//   F16  the flash fp16 core (fp16_inputs): q, k, v, dO, P and dS enter every product as f16 on
//        v_mfma_f32_32x32x16_f16, O rounded to f16; statistics, dS and accumulators fp32
//   X3   the fp32 core with every product in three bf16 MFMA passes on split operands (opt-in:
//        cmt_attn_train_fwd_bf16x3 / _bwd_bf16x3; the arithmetic of the training GEMMs, ~2^-16
//        per product), nothing rounded on the way out
// Everything else -- head pointers, DN ranges, the edge test, the softmax, the dropout hash,
// dS = P (dP - delta) and the three epilogues -- is the one body.
//
// DN mask (dn_pad > 0): key k is hidden from query q if k < dn_pad and (q >= dn_pad or
// k / dn_group != q / dn_group).  Dropout (p > 0) keeps P(q, k) with probability 1 - p by a
// counter hash of (seed, b, h, q, k), recomputed identically in the backward; the scale
// 1 / (1 - p) multiplies O, dV and dP once instead of each P.
//
// The long-key fp16 path (the cross-attention of the training step) has kernels of its own below.
#include "cmt_common.h"

#include <cstdlib>

namespace {

constexpr int D = 32;
constexpr int KT = 64;
constexpr float LOG2E = 1.4426950408889634f;

struct AP {                  // device-side copy of cmt_attn_train_args + derived values
    cmt_attn_train_args a;
    float c;                 // scale * log2(e)
    int tiles_per_split;
    float keep_scale;        // 1 / (1 - p)
    uint32_t drop_thr;       // keep iff hash >= thr
};

__device__ __forceinline__ float r16(float x) { return (float)(_Float16)x; }

// dev diagnostic bits (dev/build_exp.sh -DCMT_AT_VAR=n; the product builds 0): 2 / 4 = no dropout
// hash / no DN mask (wrong results, for timing what each costs: dev/attn_train_probe.py)
#ifndef CMT_AT_VAR
#define CMT_AT_VAR 0
#endif
// exp2 as one v_exp_f32 (exp2f adds denormal range scaling around it): the exact-f32 kernels'
// softmax arguments are <= 0 and a flushed denormal P is below every tolerance of the step
// (profiles/r6_experiments.txt r6f: 70.8 -> 66.7 us forward at the coop self-attention shape)
__device__ __forceinline__ float xexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// The DN mask without a per-element integer division: the DN groups tile [0, dn_pad) (dn_pad is a
// multiple of dn_group), so for a FIXED query q the keys it sees below dn_pad are its own group
// [lo, hi) (none when q >= dn_pad), and for a FIXED key k < dn_pad the queries that see it are
// k's group.  One division per lane; per element two or three compares.
struct DnRange {
    int lo, hi;
};
// the lane's query q: key k is hidden iff dn_hidden_key(a, r, k)
__device__ __forceinline__ DnRange dn_query_range(const cmt_attn_train_args& a, int q) {
    if (a.dn_pad <= 0 || q >= a.dn_pad) return DnRange{0, 0};
    const int lo = (q / a.dn_group) * a.dn_group;
    return DnRange{lo, min(lo + a.dn_group, a.dn_pad)};
}
__device__ __forceinline__ bool dn_hidden_key(const cmt_attn_train_args& a, const DnRange& r, int k) {
    if constexpr ((CMT_AT_VAR & 4) != 0) return false;
    return k < a.dn_pad && (k < r.lo || k >= r.hi);
}
// the lane's key k: query q is hidden from it iff dn_hidden_query(r, q)
__device__ __forceinline__ DnRange dn_key_range(const cmt_attn_train_args& a, int k) {
    if (a.dn_pad <= 0 || k >= a.dn_pad) return DnRange{INT_MIN, INT_MAX};
    const int lo = (k / a.dn_group) * a.dn_group;
    return DnRange{lo, min(lo + a.dn_group, a.dn_pad)};
}
__device__ __forceinline__ bool dn_hidden_query(const DnRange& r, int q) {
    if constexpr ((CMT_AT_VAR & 4) != 0) return false;
    return q < r.lo || q >= r.hi;
}
// key k of the tile loop is out of the problem (only in the last tile: edge) or hidden by the mask
__device__ __forceinline__ bool past_end(const cmt_attn_train_args& a, bool edge, int k) { return edge && k >= a.Nk; }

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// the dropout seed of the launch: seed (+ *seed_dev, ABI 22), resolved once per kernel into p.a.seed
__device__ __forceinline__ void resolve_seed(AP& p) {
    if (p.a.seed_dev) p.a.seed += *p.a.seed_dev;
}
// The dropout hash of (seed, b, h, q, k) in two steps: its (seed, b, h, q) part once per query (per
// lane in the forward / dQ kernels, per staged query in the dK/dV kernel), the key's part per
// element -- the per-element integer multiplies are what is left beside the 16x-rate MFMAs.
__device__ __forceinline__ uint32_t keep_row(const AP& p, int bh, int q) {
    return mix32(p.a.seed ^ mix32((uint32_t)bh * 0x9e3779b9U + (uint32_t)q));
}
__device__ __forceinline__ bool keep_col(const AP& p, uint32_t hrow, int k) {
    if constexpr ((CMT_AT_VAR & 2) != 0) return true;
    return mix32(hrow ^ (uint32_t)k * 0x85ebca6bU) >= p.drop_thr;
}
// dS = P (dP' - delta), dP' = dP of a kept element / (1 - p)
template <bool DROP>
__device__ __forceinline__ float ds_of(const AP& p, float pr, float dp, bool kept, float delta) {
    const float g = !DROP ? dp : kept ? dp * p.keep_scale : 0.f;
    return pr * (g - delta);
}

// register r of lane half lh of a 32x32 accumulator tile is row key_of(r, lh)
__device__ __forceinline__ int key_of(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// ---------------------------------------------------------------------------
// f16 / bf16 tile pieces (F16, X3 and the long-key kernels).  A 64-row tile is a row-major image
// [row][32 d] of 64-byte rows, 16-byte chunks XOR-swizzled by (row >> 2) & 3: the 16-lane groups
// of ds_read_b128 hit distinct bank slots, row reads and transposed reads both conflict-free.  A
// product whose B operand is an accumulator tile (P^T, dS^T, P, dS) takes the accumulator's own
// row order as its k order: register 8 ss + j of lane half lh is row (j & 3) + 16 ss +
// 8 (j >> 2) + 4 lh, and its A operand is read transposed from the same row-major image.
// ---------------------------------------------------------------------------
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
constexpr int RMB = 64;    // bytes per row-major LDS row (32 d)

__device__ __forceinline__ int rm_off(int row, int chunk) { return row * RMB + ((chunk ^ ((row >> 2) & 3)) << 4); }

// thread tid's 8 floats of rows r0 .. r0+63 of X (row stride rs; rows >= nrows are zero): row
// tid >> 2, columns 8 (tid & 3) .. + 7
__device__ __forceinline__ void tile_chunk(const float* X, int64_t rs, int r0, int nrows, int tid, f32x4& a, f32x4& b) {
    const int r = tid >> 2, c = tid & 3;
    a = f32x4{0.f, 0.f, 0.f, 0.f};
    b = a;
    if (r0 + r < nrows) {
        a = *(const f32x4*)(X + (int64_t)(r0 + r) * rs + 8 * c);
        b = *(const f32x4*)(X + (int64_t)(r0 + r) * rs + 8 * c + 4);
    }
}
// A fragment of rows rb*32 + (lane & 31) of a row-major image, d half kk
__device__ __forceinline__ h8_t frag_rm(const char* rm, int rb, int kk, int lane) {
    return *(const h8_t*)(rm + rm_off(rb * 32 + (lane & 31), 2 * kk + (lane >> 5)));
}
// A operand of a product over 16 rows [r0, r0 + 16) of a row-major swizzled image (the rows in
// the accumulator order of frag_acc): lane (lh, d = lane & 31) gets rows r0 + 4 lh + 0..3 and
// r0 + 8 + 4 lh + 0..3 of column d (two ds_read_b64_tr_b16, cdna_hip_programming.md T10)
__device__ __forceinline__ h8_t tr_frag(const char* img, int r0, int lane) {
    const int g = lane >> 4, lh = lane >> 5, qq = (lane & 15) >> 2, pp = lane & 3;
    const int c = 2 * (g & 1) + (pp >> 1);
    const int ra = r0 + 4 * lh + qq, rb = ra + 8;
    const char* pa = img + ra * 64 + ((c ^ ((ra >> 2) & 3)) << 4) + 8 * (pp & 1);
    const char* pb = img + rb * 64 + ((c ^ ((rb >> 2) & 3)) << 4) + 8 * (pp & 1);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((CMT_LDS s16v4_lds*)pa);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((CMT_LDS s16v4_lds*)pb);
    s16x8 v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
    v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    return __builtin_bit_cast(h8_t, v);
}
// B fragment from accumulator registers 8 ss .. 8 ss + 7 (rounded to f16)
__device__ __forceinline__ h8_t frag_acc(const f32x16& x, int ss) {
    h8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)x[8 * ss + j];
    return v;
}
__device__ __forceinline__ f32x16 mma16(h8_t a, h8_t b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 as_bf16(h8_t v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ void split_x3(float x, bf16_t& hi, bf16_t& lo) {
    hi = (bf16_t)x;
    lo = (bf16_t)(x - (float)hi);
}

// ---------------------------------------------------------------------------
// The arithmetic policies.  stage(lds, X, rs, r0, nrows, tid): rows r0 .. r0+63 of X into a tile
// (256 threads); load_own(row, lh): a lane's own row of 32 fp32 values as B fragments;
// rows_x_own: acc += tile rows 32 rb + (lane & 31) . own row (lane = the own row's index);
// tr_x_acc: acc^T[d][col] += sum_k Z[k][d] W[k][col], Z the tile's rows 32 rb .. + 31 and W an
// accumulator tile (lane = col, register r <-> k = key_of(r, lh)).
// ---------------------------------------------------------------------------
struct F32 {
    static constexpr int LDK = 36;                // padded f32 LDS row
    static constexpr int TILE = KT * LDK * 4;
    struct Own {
        f32x4 f[4];                               // d = 16 lh + 4 i + j
    };
    static __device__ __forceinline__ void stage(char* lds, const float* X, int64_t rs, int r0, int nrows, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx >> 3, c = (idx & 7) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < nrows) v = *(const f32x4*)(X + (int64_t)(r0 + r) * rs + c);
            *(f32x4*)((float*)lds + r * LDK + c) = v;
        }
    }
    static __device__ __forceinline__ Own load_own(const float* row, int lh) {
        Own o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o.f[i] = *(const f32x4*)(row + 16 * lh + 4 * i);
        return o;
    }
    static __device__ __forceinline__ void rows_x_own(const char* lds, int rb, int lane, const Own& own, f32x16& acc) {
        const float* xrow = (const float*)lds + (rb * 32 + (lane & 31)) * LDK + 16 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 xv = *(const f32x4*)(xrow + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j], own.f[i][j], acc, 0, 0, 0);
        }
    }
    static __device__ __forceinline__ void tr_x_acc(const char* lds, int rb, int lane, const f32x16& w, f32x16& acc) {
        const float* z = (const float*)lds + rb * 32 * LDK;
        const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z[key_of(r, lh) * LDK + lr], w[r], acc, 0, 0, 0);
    }
    static __device__ __forceinline__ float round_o(float x) { return x; }
    static __device__ __forceinline__ float ex2(float x) { return xexp2(x); }
};

struct F16 {
    static constexpr int TILE = KT * RMB;         // one row-major f16 image
    struct Own {
        h8_t f[2];                                // d = 16 kk + 8 lh + j
    };
    static __device__ __forceinline__ void stage(char* lds, const float* X, int64_t rs, int r0, int nrows, int tid) {
        f32x4 a, b;
        tile_chunk(X, rs, r0, nrows, tid, a, b);
        h8_t hv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            hv[j] = (_Float16)a[j];
            hv[4 + j] = (_Float16)b[j];
        }
        *(h8_t*)(lds + rm_off(tid >> 2, tid & 3)) = hv;
    }
    static __device__ __forceinline__ Own load_own(const float* row, int lh) {
        Own o;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const f32x4 a = *(const f32x4*)(row + 16 * kk + 8 * lh), b = *(const f32x4*)(row + 16 * kk + 8 * lh + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o.f[kk][j] = (_Float16)a[j];
                o.f[kk][4 + j] = (_Float16)b[j];
            }
        }
        return o;
    }
    static __device__ __forceinline__ void rows_x_own(const char* lds, int rb, int lane, const Own& own, f32x16& acc) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) acc = mma16(frag_rm(lds, rb, kk, lane), own.f[kk], acc);
    }
    // P and dS are rounded to f16 here, as they enter the product
    static __device__ __forceinline__ void tr_x_acc(const char* lds, int rb, int lane, const f32x16& w, f32x16& acc) {
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) acc = mma16(tr_frag(lds, rb * 32 + 16 * ss, lane), frag_acc(w, ss), acc);
    }
    static __device__ __forceinline__ float round_o(float x) { return r16(x); }
    static __device__ __forceinline__ float ex2(float x) { return exp2f(x); }
};

// Every fp32 operand is split x = hi + lo, hi = bf16(x) (RNE), lo = bf16(x - hi) -- bf16 keeps the
// fp32 exponent, so gradient-sized dO and dS split without underflow -- and every product runs as
// lo*hi + hi*lo + hi*hi (small terms first, lo*lo dropped) on v_mfma_f32_32x32x16_bf16, fp32
// accumulate (train.hip gemm_x3_kernel).  Q, K, V and dO are split as they are staged (two images
// per tile), a lane's own row and the accumulator tiles P / dS (fp32) in registers.
struct X3 {
    static constexpr int IMG = KT * RMB;          // the lo image follows the hi one
    static constexpr int TILE = 2 * IMG;
    struct Own {
        bf16x8 hi[2], lo[2];                      // d = 16 kk + 8 lh + j
    };
    // c += A B in three passes, small terms first
    static __device__ __forceinline__ f32x16 mma(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x16 c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void stage(char* lds, const float* X, int64_t rs, int r0, int nrows, int tid) {
        f32x4 a, b;
        tile_chunk(X, rs, r0, nrows, tid, a, b);
        bf16x8 hv, lv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bf16_t h, l;
            split_x3(a[j], h, l);
            hv[j] = h; lv[j] = l;
            split_x3(b[j], h, l);
            hv[4 + j] = h; lv[4 + j] = l;
        }
        *(bf16x8*)(lds + rm_off(tid >> 2, tid & 3)) = hv;
        *(bf16x8*)(lds + IMG + rm_off(tid >> 2, tid & 3)) = lv;
    }
    static __device__ __forceinline__ Own load_own(const float* row, int lh) {
        Own o;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const f32x4 a = *(const f32x4*)(row + 16 * kk + 8 * lh), b = *(const f32x4*)(row + 16 * kk + 8 * lh + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16_t h, l;
                split_x3(a[j], h, l);
                o.hi[kk][j] = h; o.lo[kk][j] = l;
                split_x3(b[j], h, l);
                o.hi[kk][4 + j] = h; o.lo[kk][4 + j] = l;
            }
        }
        return o;
    }
    static __device__ __forceinline__ void rows_x_own(const char* lds, int rb, int lane, const Own& own, f32x16& acc) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            acc = mma(as_bf16(frag_rm(lds, rb, kk, lane)), as_bf16(frag_rm(lds + IMG, rb, kk, lane)), own.hi[kk],
                      own.lo[kk], acc);
    }
    static __device__ __forceinline__ void tr_x_acc(const char* lds, int rb, int lane, const f32x16& w, f32x16& acc) {
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            bf16x8 wh, wl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bf16_t h, l;
                split_x3(w[8 * ss + j], h, l);
                wh[j] = h; wl[j] = l;
            }
            const int r0 = rb * 32 + 16 * ss;
            acc = mma(as_bf16(tr_frag(lds, r0, lane)), as_bf16(tr_frag(lds + IMG, r0, lane)), wh, wl, acc);
        }
    }
    static __device__ __forceinline__ float round_o(float x) { return x; }
    static __device__ __forceinline__ float ex2(float x) { return xexp2(x); }
};

// ---------------------------------------------------------------------------
// The three passes
// ---------------------------------------------------------------------------
struct Heads {   // head (b, h) of Q, K, V and dO / O
    const float *Q, *K, *V, *dO;
};
__device__ __forceinline__ Heads head_ptrs(const cmt_attn_train_args& a, int b, int h) {
    return Heads{a.Q + (int64_t)b * a.q_bs + (int64_t)h * a.q_hs, a.K + (int64_t)b * a.k_bs + (int64_t)h * a.k_hs,
                 a.V + (int64_t)b * a.v_bs + (int64_t)h * a.v_hs, a.dO + (int64_t)b * a.o_bs + (int64_t)h * a.o_hs};
}
__device__ __forceinline__ void zero16(f32x16& x) {
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = 0.f;
}

template <class A, bool MASK, bool DROP>
__global__ __launch_bounds__(256) void fwd_kernel(AP p) {
    resolve_seed(p);
    const cmt_attn_train_args& a = p.a;
    __shared__ __attribute__((aligned(16))) char Ks[A::TILE];
    __shared__ __attribute__((aligned(16))) char Vs[A::TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, split = blockIdx.z;
    const Heads hd = head_ptrs(a, b, h);
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const DnRange dnr = dn_query_range(a, q);
    const uint32_t hrow = keep_row(p, bh, q);
    const int qc = min(q, a.Nq - 1);
    const typename A::Own qf = A::load_own(hd.Q + (int64_t)qc * a.q_rs, lh);
    const int ntiles = (a.Nk + KT - 1) / KT;
    const int t0 = split * p.tiles_per_split, t1 = min(ntiles, t0 + p.tiles_per_split);
    f32x16 o;
    zero16(o);
    float m_run = -__builtin_inff(), l_run = 0.f;
    for (int t = t0; t < t1; ++t) {
        __syncthreads();
        A::stage(Ks, hd.K, a.k_rs, t * KT, a.Nk, tid);
        A::stage(Vs, hd.V, a.v_rs, t * KT, a.Nk, tid);
        __syncthreads();
        const bool edge = (t + 1) * KT > a.Nk;
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            zero16(s[kb]);
            A::rows_x_own(Ks, kb, lane, qf, s[kb]);                        // S^T  (lane = query)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = t * KT + kb * 32 + key_of(r, lh);
                s[kb][r] = (past_end(a, edge, k) || (MASK && dn_hidden_key(a, dnr, k))) ? -__builtin_inff() : s[kb][r] * p.c;
            }
        }
        float mt = -__builtin_inff();
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[kb][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);
        const float m_use = m_new == -__builtin_inff() ? 0.f : m_new;   // fully masked so far
        const float alpha = A::ex2(m_run - m_use);
        float ls = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = A::ex2(s[kb][r] - m_use);
                ls += e;                                                   // the statistics see every P
                const bool kp = !DROP || keep_col(p, hrow, t * KT + kb * 32 + key_of(r, lh));
                s[kb][r] = kp ? e : 0.f;
            }
        l_run = l_run * alpha + ls;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) A::tr_x_acc(Vs, kb, lane, s[kb], o);   // O^T += V^T P^T
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    if (DROP) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= p.keep_scale;
    }
    if (q >= a.Nq) return;
    if (a.kv_splits <= 1) {
        const float inv = 1.f / l_tot;
        float* Ob = a.O + (int64_t)b * a.o_bs + (int64_t)h * a.o_hs + (int64_t)q * a.o_rs;
#pragma unroll
        for (int r = 0; r < 16; ++r) Ob[key_of(r, lh)] = A::round_o(o[r] * inv);
        if (lh == 0) a.LSE[(int64_t)bh * a.Nq + q] = m_run + log2f(l_tot);
    } else {   // this split's partial (train_combine_kernel)
        float* ws = (float*)a.workspace;
        const int64_t rows = (int64_t)a.B * a.H * a.Nq;
        const int64_t row = (int64_t)split * rows + (int64_t)bh * a.Nq + q;
        float* Op = ws + row * D;
#pragma unroll
        for (int r = 0; r < 16; ++r) Op[key_of(r, lh)] = o[r];
        if (lh == 0) {
            ws[(int64_t)a.kv_splits * rows * D + row] = m_run;
            ws[(int64_t)a.kv_splits * rows * (D + 1) + row] = l_tot;
        }
    }
}

// dQ: waves own 32 queries; key tiles [t0, t1) of this split; f32 atomics into dQ when split
template <class A, bool MASK, bool DROP>
__global__ __launch_bounds__(256) void dq_kernel(AP p) {
    resolve_seed(p);
    const cmt_attn_train_args& a = p.a;
    __shared__ __attribute__((aligned(16))) char Ks[A::TILE];
    __shared__ __attribute__((aligned(16))) char Vs[A::TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, split = blockIdx.z;
    const Heads hd = head_ptrs(a, b, h);
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const DnRange dnr = dn_query_range(a, q);
    const uint32_t hrow = keep_row(p, bh, q);
    const int qc = min(q, a.Nq - 1);
    const typename A::Own qf = A::load_own(hd.Q + (int64_t)qc * a.q_rs, lh);
    const typename A::Own df = A::load_own(hd.dO + (int64_t)qc * a.o_rs, lh);
    const float lse = a.LSE[(int64_t)bh * a.Nq + qc];
    const float dl = a.delta[(int64_t)bh * a.Nq + qc];
    const int ntiles = (a.Nk + KT - 1) / KT;
    const int t0 = split * p.tiles_per_split, t1 = min(ntiles, t0 + p.tiles_per_split);
    f32x16 dq;
    zero16(dq);
    for (int t = t0; t < t1; ++t) {
        __syncthreads();
        A::stage(Ks, hd.K, a.k_rs, t * KT, a.Nk, tid);
        A::stage(Vs, hd.V, a.v_rs, t * KT, a.Nk, tid);
        __syncthreads();
        const bool edge = (t + 1) * KT > a.Nk;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 s, dp;
            zero16(s);
            zero16(dp);
            A::rows_x_own(Ks, kb, lane, qf, s);                            // S^T  (lane = query)
            A::rows_x_own(Vs, kb, lane, df, dp);                           // dP^T = V dO^T
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = t * KT + kb * 32 + key_of(r, lh);
                const float pr = (past_end(a, edge, k) || (MASK && dn_hidden_key(a, dnr, k))) ? 0.f : A::ex2(s[r] * p.c - lse);
                s[r] = ds_of<DROP>(p, pr, dp[r], !DROP || keep_col(p, hrow, k), dl);   // dS^T
            }
            A::tr_x_acc(Ks, kb, lane, s, dq);                              // dQ^T += K^T dS^T
        }
    }
    if (q >= a.Nq) return;
    float* dQb = a.dQ + (int64_t)b * a.q_bs + (int64_t)h * a.q_hs + (int64_t)q * a.q_rs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = dq[r] * a.scale;
        if (a.kv_splits > 1) atomicAdd(dQb + key_of(r, lh), v);
        else dQb[key_of(r, lh)] = v;
    }
}

// dK, dV: waves own 32 keys; loop over 64-query tiles (Q, dO, LSE2, delta and the queries' half of
// the dropout hash in LDS), query tiles [z qt_per, (z + 1) qt_per) of split z = blockIdx.z (f32
// atomics into zeroed dK / dV when split: the self-attention's ~1 100 keys alone are 9 x 8
// workgroups)
template <class A, bool MASK, bool DROP>
__global__ __launch_bounds__(256) void dkv_kernel(AP p, int qt_per) {
    resolve_seed(p);
    const cmt_attn_train_args& a = p.a;
    __shared__ __attribute__((aligned(16))) char Qs[A::TILE];
    __shared__ __attribute__((aligned(16))) char Ds[A::TILE];   // dO
    __shared__ float Ls[KT], Dl[KT];
    __shared__ uint32_t Hq[KT];                                 // keep_row of the tile's queries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const Heads hd = head_ptrs(a, b, h);
    const int k = blockIdx.x * 128 + wave * 32 + lr;
    const DnRange dnr = dn_key_range(a, k);
    const int kc = min(k, a.Nk - 1);
    const typename A::Own kf = A::load_own(hd.K + (int64_t)kc * a.k_rs, lh);
    const typename A::Own vf = A::load_own(hd.V + (int64_t)kc * a.v_rs, lh);
    f32x16 dk, dv;
    zero16(dk);
    zero16(dv);
    const int nqt = (a.Nq + KT - 1) / KT;
    const int tq0 = blockIdx.z * qt_per, tq1 = min(nqt, tq0 + qt_per);
    for (int t = tq0; t < tq1; ++t) {
        __syncthreads();
        A::stage(Qs, hd.Q, a.q_rs, t * KT, a.Nq, tid);
        A::stage(Ds, hd.dO, a.o_rs, t * KT, a.Nq, tid);
        if (tid < KT) {
            const int qq = min(t * KT + tid, a.Nq - 1);
            Ls[tid] = a.LSE[(int64_t)bh * a.Nq + qq];
            Dl[tid] = a.delta[(int64_t)bh * a.Nq + qq];
            if (DROP) Hq[tid] = keep_row(p, bh, t * KT + tid);
        }
        __syncthreads();
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            f32x16 s, dp;
            zero16(s);
            zero16(dp);
            A::rows_x_own(Qs, qb, lane, kf, s);                            // S = Q K^T (lane = key)
            A::rows_x_own(Ds, qb, lane, vf, dp);                           // dP = dO V^T
            f32x16 pd;                                                     // P, dropped (dV operand; scale later)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = qb * 32 + key_of(r, lh), qq = t * KT + qi;
                const bool valid = qq < a.Nq && k < a.Nk && !(MASK && dn_hidden_query(dnr, qq));
                const float pr = valid ? A::ex2(s[r] * p.c - Ls[qi]) : 0.f;
                const bool kp = !DROP || keep_col(p, Hq[qi], k);
                pd[r] = kp ? pr : 0.f;
                s[r] = ds_of<DROP>(p, pr, dp[r], kp, Dl[qi]);              // dS
            }
            A::tr_x_acc(Ds, qb, lane, pd, dv);                             // dV^T += dO^T P
            A::tr_x_acc(Qs, qb, lane, s, dk);                              // dK^T += Q^T dS
        }
    }
    if (k >= a.Nk) return;
    float* dKb = a.dK + (int64_t)b * a.k_bs + (int64_t)h * a.k_hs + (int64_t)k * a.k_rs;
    float* dVb = a.dV + (int64_t)b * a.v_bs + (int64_t)h * a.v_hs + (int64_t)k * a.v_rs;
    const float vs = DROP ? p.keep_scale : 1.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (gridDim.z > 1) {
            atomicAdd(dKb + key_of(r, lh), dk[r] * a.scale);
            atomicAdd(dVb + key_of(r, lh), dv[r] * vs);
        } else {
            dKb[key_of(r, lh)] = dk[r] * a.scale;
            dVb[key_of(r, lh)] = dv[r] * vs;
        }
    }
}

__global__ __launch_bounds__(256) void train_combine_kernel(AP p) {
    const cmt_attn_train_args& a = p.a;
    const int64_t rows = (int64_t)a.B * a.H * a.Nq;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * D) return;
    const int64_t row = i / D;
    const int d = (int)(i - row * D);
    const float* ws = (const float*)a.workspace;
    const int S = a.kv_splits;
    float M = -__builtin_inff();
    for (int s = 0; s < S; ++s) {
        const float l = ws[(int64_t)S * rows * (D + 1) + s * rows + row];
        if (l > 0.f) M = fmaxf(M, ws[(int64_t)S * rows * D + s * rows + row]);
    }
    float num = 0.f, den = 0.f;
    for (int s = 0; s < S; ++s) {
        const float l = ws[(int64_t)S * rows * (D + 1) + s * rows + row];
        if (!(l > 0.f)) continue;
        const float w = xexp2(ws[(int64_t)S * rows * D + s * rows + row] - M);
        num += w * ws[(s * rows + row) * D + d];
        den += w * l;
    }
    const int bh = (int)(row / a.Nq), q = (int)(row - (int64_t)bh * a.Nq);
    const int b = bh / a.H, h = bh - b * a.H;
    const float v = num / den;
    a.O[(int64_t)b * a.o_bs + (int64_t)h * a.o_hs + (int64_t)q * a.o_rs + d] = a.fp16_inputs ? r16(v) : v;
    if (d == 0) a.LSE[row] = M + log2f(den);
}

// delta[b,h,q] = sum_d dO * O
__global__ __launch_bounds__(256) void train_delta_kernel(AP p) {
    const cmt_attn_train_args& a = p.a;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)a.B * a.H * a.Nq) return;
    const int bh = (int)(row / a.Nq), q = (int)(row - (int64_t)bh * a.Nq);
    const int b = bh / a.H, h = bh - b * a.H;
    const int64_t off = (int64_t)b * a.o_bs + (int64_t)h * a.o_hs + (int64_t)q * a.o_rs;
    float v = lane < D ? a.dO[off + lane] * a.O[off + lane] : 0.f;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) a.delta[row] = v;
}

// ---------------------------------------------------------------------------
// Long-key fp16 path (the cross-attention of the training step: FlashMHA's fp16
// core, no DN mask, no dropout; Nk of 36 400 / 44 400 keys against ~1 100
// queries).  The operands are first rounded to f16 ONCE into head-split copies
// [B][H][N][32] (to16_kernel, with the K projection's per-64-key max |k|^2 for
// the bounded forward), then:
//   forward   the inference core (attention.hip attn_pb2_kernel + split combine,
//             cmt_attn_fwd_lse) with the row statistic;
//   dK / dV   train16_dkv2_kernel: 8 waves x 32 keys, the head's whole Q and dO
//             (f16, <= 1 152 queries) resident in LDS -- no per-tile staging or
//             barrier; S and dP with the key on the lane, so P and dS are the B
//             operands of dV^T += dO^T P and dK^T += Q^T dS, whose A operands are
//             ds_read_b64_tr_b16 transposed reads of the same row-major images;
//   dQ        train16_dq2_kernel: 8 waves x 32 queries, K / V tiles by LDS-DMA
//             into a 4-slot ring (one barrier per tile), S^T and dP^T with the
//             query on the lane, dQ^T += K^T dS^T on transposed reads of the K
//             image, key splits summed by f32 atomics.
// ---------------------------------------------------------------------------
constexpr int NQ_RES = 1152;   // queries resident in LDS (dkv2): 2 x 72 KB images + statistics
constexpr int DQ_RING = 4;

// f16 head-split copy Y[(b H + h) N + n][32] of X[b bs + h hs + n rs + d]; with kmax2, also
// kmax2[e * H + h] = max over rows r = b N + n in [64 e, 64 e + 64) of |Y row|^2 (the rounded
// values: the bound of the forward's bounded offsets).  Block (e, h): 64 rows x 4 threads.
__global__ __launch_bounds__(256) void to16_kernel(const float* X, int64_t bs, int64_t hs, int64_t rs, int B, int H,
                                                   int N, f16_t* Y, float* kmax2) {
    const int e = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int64_t r = (int64_t)e * 64 + (tid >> 2);
    const int d0 = (tid & 3) * 8;
    float ss = 0.f;
    if (r < (int64_t)B * N) {
        const int b = (int)(r / N), n = (int)(r - (int64_t)b * N);
        const float* x = X + (int64_t)b * bs + (int64_t)h * hs + (int64_t)n * rs + d0;
        const f32x4 u = *(const f32x4*)x, w = *(const f32x4*)(x + 4);
        h8_t v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (f16_t)u[j];
            v[4 + j] = (f16_t)w[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += (float)v[j] * (float)v[j];
        *(h8_t*)(Y + (((int64_t)b * H + h) * N + n) * D + d0) = v;
    }
    if (kmax2 == nullptr) return;
    ss += __shfl_xor(ss, 1);
    ss += __shfl_xor(ss, 2);
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) ss = fmaxf(ss, __shfl_xor(ss, o));
    __shared__ float wm[4];
    if ((tid & 63) == 0) wm[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) kmax2[(int64_t)e * H + h] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

__global__ __launch_bounds__(512, 1) void train16_dkv2_kernel(AP p, const f16_t* Q16, const f16_t* D16,
                                                            const f16_t* K16, const f16_t* V16, int nqp) {
    const cmt_attn_train_args& a = p.a;
    __shared__ __attribute__((aligned(16))) char Qs[NQ_RES * 64];
    __shared__ __attribute__((aligned(16))) char Ds[NQ_RES * 64];
    __shared__ __attribute__((aligned(16))) float Ls[NQ_RES];
    __shared__ __attribute__((aligned(16))) float Dl[NQ_RES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const f16_t* Qh = Q16 + (int64_t)bh * a.Nq * D;
    const f16_t* Dh = D16 + (int64_t)bh * a.Nq * D;
    // the head's Q and dO (padded rows zero) and statistics (padded rows: P = 0)
    for (int i = tid; i < nqp * 4; i += 512) {
        const int r = i >> 2, c = i & 3;
        h8_t qv = {}, dv = {};
        if (r < a.Nq) {
            qv = *(const h8_t*)(Qh + (int64_t)r * D + 8 * c);
            dv = *(const h8_t*)(Dh + (int64_t)r * D + 8 * c);
        }
        *(h8_t*)(Qs + rm_off(r, c)) = qv;
        *(h8_t*)(Ds + rm_off(r, c)) = dv;
    }
    for (int i = tid; i < nqp; i += 512) {
        Ls[i] = i < a.Nq ? a.LSE[(int64_t)bh * a.Nq + i] : __builtin_inff();
        Dl[i] = i < a.Nq ? a.delta[(int64_t)bh * a.Nq + i] : 0.f;
    }
    // this lane's key row of K and V as the B operands (k = d = 16 kk + 8 lh + j)
    const int k = blockIdx.x * 256 + wave * 32 + lr;
    const int kc = min(k, a.Nk - 1);
    const f16_t* Kr = K16 + ((int64_t)bh * a.Nk + kc) * D;
    const f16_t* Vr = V16 + ((int64_t)bh * a.Nk + kc) * D;
    h8_t kf[2], vf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        kf[kk] = *(const h8_t*)(Kr + 16 * kk + 8 * lh);
        vf[kk] = *(const h8_t*)(Vr + 16 * kk + 8 * lh);
    }
    __syncthreads();
    f32x16 dk, dv;
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;
    const float c = p.c;
    for (int q0 = 0; q0 < nqp; q0 += 32) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int o = rm_off(q0 + lr, 2 * kk + lh);
            s = mma16(*(const h8_t*)(Qs + o), kf[kk], s);      // S = Q K^T (lane = key)
            dp = mma16(*(const h8_t*)(Ds + o), vf[kk], dp);    // dP = dO V^T
        }
        // register r of lane half lh is query q0 + 8 (r >> 2) + 4 lh + (r & 3)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 L = *(const f32x4*)(Ls + q0 + 8 * g + 4 * lh);
            const f32x4 Dv = *(const f32x4*)(Dl + q0 + 8 * g + 4 * lh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                const float pr = __builtin_amdgcn_exp2f(s[r] * c - L[e]);
                s[r] = pr;                                        // P
                dp[r] = pr * (dp[r] - Dv[e]);                     // dS
            }
        }
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            dv = mma16(tr_frag(Ds, q0 + 16 * ss, lane), frag_acc(s, ss), dv);    // dV^T += dO^T P
            dk = mma16(tr_frag(Qs, q0 + 16 * ss, lane), frag_acc(dp, ss), dk);   // dK^T += Q^T dS
        }
    }
    if (k >= a.Nk) return;
    float* dKb = a.dK + (int64_t)b * a.k_bs + (int64_t)h * a.k_hs + (int64_t)k * a.k_rs;
    float* dVb = a.dV + (int64_t)b * a.v_bs + (int64_t)h * a.v_hs + (int64_t)k * a.v_rs;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *(f32x4*)(dKb + 8 * g + 4 * lh) = f32x4{dk[4 * g] * a.scale, dk[4 * g + 1] * a.scale, dk[4 * g + 2] * a.scale,
                                                dk[4 * g + 3] * a.scale};
        *(f32x4*)(dVb + 8 * g + 4 * lh) = f32x4{dv[4 * g], dv[4 * g + 1], dv[4 * g + 2], dv[4 * g + 3]};
    }
}

__device__ __forceinline__ void dq2_wait(int n) {   // n = this wave's DMA pieces allowed in flight
    if (n >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (n == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One block of 32 queries per wave, 256 queries per workgroup (two blocks per wave halve the LDS
// reads per query but needed 240 VGPRs, two waves per SIMD instead of four: 238 vs 206 us, r4v)
__global__ __launch_bounds__(512) void train16_dq2_kernel(AP p, const f16_t* Q16, const f16_t* D16, const f16_t* K16,
                                                          const f16_t* V16) {
    const cmt_attn_train_args& a = p.a;
    __shared__ __attribute__((aligned(16))) char ring[DQ_RING * 2 * KT * 64];   // [slot][K | V][64 rows][64 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H, split = blockIdx.z;
    const int q = blockIdx.x * 256 + wave * 32 + lr;
    const int qc = min(q, a.Nq - 1);
    const f16_t* Qr = Q16 + ((int64_t)bh * a.Nq + qc) * D;
    const f16_t* Dr = D16 + ((int64_t)bh * a.Nq + qc) * D;
    h8_t qf[2], df[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        qf[kk] = *(const h8_t*)(Qr + 16 * kk + 8 * lh);
        df[kk] = *(const h8_t*)(Dr + 16 * kk + 8 * lh);
    }
    const float L = a.LSE[(int64_t)bh * a.Nq + qc];
    const float dl = a.delta[(int64_t)bh * a.Nq + qc];
    const int ntiles = (a.Nk + KT - 1) / KT;
    const int t0 = split * p.tiles_per_split, t1 = min(ntiles, t0 + p.tiles_per_split);
    // the 8 1-KB pieces of a tile (K rows 16 c .. 16 c + 15 for c < 4, then V): piece w by wave w;
    // a lane's LDS destination is lane-linear, the swizzle sits on the source chunk
    const int mat = wave >> 2, piece = wave & 3;
    const int prow = 16 * piece + (lane >> 2);
    const f16_t* src0 = (mat ? V16 : K16) + (int64_t)bh * a.Nk * D + 8 * ((lane & 3) ^ ((prow >> 2) & 3));
    char* dst0 = ring + mat * KT * 64 + piece * 1024;
    const int prow_l = lane >> 2;
    int issued = t0;
    auto issue_upto = [&](int n) {
        const int e = min(n, t1);
        while (issued < e) {
            const int key = min(issued * KT + 16 * piece + prow_l, a.Nk - 1);
            glds16(src0 + (int64_t)key * D, dst0 + (issued % DQ_RING) * 2 * KT * 64);
            ++issued;
        }
    };
    issue_upto(t0 + DQ_RING - 1);
    f32x16 dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] = 0.f;
    const float c = p.c;
    for (int t = t0; t < t1; ++t) {
        dq2_wait(issued - t - 1);
        barrier_mem();                                  // tile t landed for every wave; tile t-1 consumed
        issue_upto(t + DQ_RING);
        const char* Ks = ring + (t % DQ_RING) * 2 * KT * 64;
        const char* Vs = Ks + KT * 64;
        const bool edge = (t + 1) * KT > a.Nk;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            h8_t kfr[2], vfr[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int o = rm_off(kb * 32 + lr, 2 * kk + lh);
                kfr[kk] = *(const h8_t*)(Ks + o);
                vfr[kk] = *(const h8_t*)(Vs + o);
            }
            f32x16 sp, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) sp[r] = dp[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                sp = mma16(kfr[kk], qf[kk], sp);      // S^T = K Q^T (lane = query)
                dp = mma16(vfr[kk], df[kk], dp);      // dP^T = V dO^T
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float pr = __builtin_amdgcn_exp2f(sp[r] * c - L);
                if (edge && t * KT + kb * 32 + key_of(r, lh) >= a.Nk) pr = 0.f;
                sp[r] = pr * (dp[r] - dl);              // dS^T
            }
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) dq = mma16(tr_frag(Ks, kb * 32 + 16 * ss, lane), frag_acc(sp, ss), dq);
        }
    }
    if (q >= a.Nq) return;
    float* dQb = a.dQ + (int64_t)b * a.q_bs + (int64_t)h * a.q_hs + (int64_t)q * a.q_rs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = dq[r] * a.scale;
        if (gridDim.z > 1) atomicAdd(dQb + key_of(r, lh), v);
        else dQb[key_of(r, lh)] = v;
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
AP make_ap(const cmt_attn_train_args& a, int splits) {
    AP p;
    p.a = a;
    p.a.kv_splits = splits;
    p.c = a.scale * LOG2E;
    const int ntiles = (a.Nk + KT - 1) / KT;
    p.tiles_per_split = cdiv(ntiles, splits);
    p.keep_scale = a.dropout_p > 0.f ? 1.f / (1.f - a.dropout_p) : 1.f;
    const double thr = (double)a.dropout_p * 4294967296.0;
    p.drop_thr = thr >= 4294967295.0 ? 0xffffffffU : (uint32_t)thr;
    return p;
}

int train_splits(const cmt_attn_train_args& a) {
    if (a.kv_splits > 0) return a.kv_splits;
    const int ntiles = (a.Nk + KT - 1) / KT;
    const int base = cdiv(a.Nq, 128) * a.B * a.H;
    int s = 1;
    while (base * s < 512 && ntiles / (2 * s) >= 4) s *= 2;
    return s;
}

// the forward's split partials: O, m and l per split and row
int64_t split_ws_bytes(const cmt_attn_train_args& a) {
    const int s = train_splits(a);
    if (s <= 1) return 0;
    return (int64_t)s * a.B * a.H * a.Nq * (D + 2) * (int64_t)sizeof(float);
}

int check_args(const cmt_attn_train_args& a, const char* who) {
    CMT_REQUIRE(a.B > 0 && a.H > 0 && a.Nq > 0 && a.Nk > 0, std::string(who) + ": empty problem");
    CMT_REQUIRE(a.Q && a.K && a.V && a.O && a.LSE, std::string(who) + ": null pointer");
    CMT_REQUIRE(a.q_rs % 4 == 0 && a.k_rs % 4 == 0 && a.v_rs % 4 == 0 && a.o_rs % 4 == 0 && a.q_hs % 4 == 0 &&
                a.k_hs % 4 == 0 && a.v_hs % 4 == 0 && a.q_bs % 4 == 0 && a.k_bs % 4 == 0 && a.v_bs % 4 == 0,
                std::string(who) + ": strides must keep 16-byte rows");
    CMT_REQUIRE(a.dn_pad <= 0 || a.dn_group > 0, std::string(who) + ": dn_group must be > 0 with dn_pad");
    CMT_REQUIRE(a.dropout_p >= 0.f && a.dropout_p < 1.f, std::string(who) + ": dropout_p must be in [0, 1)");
    return 0;
}

// ---- the long-key fp16 path: applicability and workspace layout
bool fast_path(const cmt_attn_train_args& a) {
    return a.fp16_inputs && a.dn_pad <= 0 && !(a.dropout_p > 0.f) && a.Nk >= 4096 && a.Nq > 128 &&
           a.Nq <= NQ_RES && a.o_hs == D && a.kv_splits <= 0;
}

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// forward key splits: one round of one-per-CU workgroups (the ping-pong kernel holds a CU); at
// ~1 100 queries the inference core's automatic choice (8 splits, 320 workgroups) ran two rounds
int fwd_splits(const cmt_attn_train_args& a) { return max(1, min(16, 256 / (cdiv(a.Nq, 256) * a.B * a.H))); }

struct FastWs {   // byte offsets into the workspace
    int64_t q16, k16, v16, d16, kmax, attn, total;
};

FastWs fast_ws(const cmt_attn_train_args& a) {
    FastWs w;
    const int64_t qn = (int64_t)a.B * a.H * a.Nq * D * 2, kn = (int64_t)a.B * a.H * a.Nk * D * 2;
    w.q16 = 0;
    w.k16 = align256(w.q16 + qn);
    w.v16 = align256(w.k16 + kn);
    w.d16 = align256(w.v16 + kn);
    w.kmax = align256(w.d16 + qn);
    w.attn = align256(w.kmax + cdiv64((int64_t)a.B * a.Nk, 64) * a.H * 4);
    cmt_attn_args g = {};
    g.B = a.B; g.H = a.H; g.Nq = a.Nq; g.Nk = a.Nk; g.dtype = CMT_F16;
    g.kv_splits = fwd_splits(a);
    w.total = align256(w.attn + cmt_attn_workspace_bytes(&g));
    return w;
}

void to16(const float* X, int64_t bs, int64_t hs, int64_t rs, int B, int H, int N, f16_t* Y, float* kmax,
          hipStream_t s) {
    to16_kernel<<<dim3((unsigned)cdiv64((int64_t)B * N, 64), (unsigned)H), 256, 0, s>>>(X, bs, hs, rs, B, H, N, Y,
                                                                                        kmax);
}

// Zeroes the [N x 32] rows of every (b, h) of a strided head-split fp32 view: one launch instead
// of a 2-D memset per (b, h)
__global__ __launch_bounds__(256) void zero_heads_kernel(float* X, int64_t bs, int64_t hs, int64_t rs, int H, int N,
                                                         int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i >> 5;          // (b, h, n) row, D = 32 floats each
        const int n = (int)(r % N);
        const int64_t bh = r / N;
        X[(bh / H) * bs + (bh % H) * hs + n * rs + (i & 31)] = 0.f;
    }
}

// Zeroes a gradient that a split pass accumulates by atomics (dQ / dK / dV, a head-split view of
// [B][N][H * 32]): one memset when the view is the whole dense tensor, the kernel above otherwise
int zero_grad(float* X, int64_t bs, int64_t hs, int64_t rs, int B, int H, int N, hipStream_t s, const char* who) {
    const int64_t total = (int64_t)B * H * N * D;
    if (hs == D && rs == (int64_t)H * D && bs == (int64_t)N * H * D) {
        CMT_REQUIRE(hipMemsetAsync(X, 0, (size_t)total * sizeof(float), s) == hipSuccess,
                    std::string(who) + ": gradient zeroing failed");
    } else {
        zero_heads_kernel<<<(unsigned)std::min<int64_t>(cdiv64(total, 256), 2048), 256, 0, s>>>(X, bs, hs, rs, H, N,
                                                                                                 total);
    }
    return 0;
}

// the <MASK, DROP> instantiations of the three passes in arithmetic A, indexed by flags()
template <class A>
struct Pass {
    static constexpr void (*fwd[4])(AP) = {fwd_kernel<A, false, false>, fwd_kernel<A, false, true>,
                                           fwd_kernel<A, true, false>, fwd_kernel<A, true, true>};
    static constexpr void (*dq[4])(AP) = {dq_kernel<A, false, false>, dq_kernel<A, false, true>,
                                          dq_kernel<A, true, false>, dq_kernel<A, true, true>};
    static constexpr void (*dkv[4])(AP, int) = {dkv_kernel<A, false, false>, dkv_kernel<A, false, true>,
                                                dkv_kernel<A, true, false>, dkv_kernel<A, true, true>};
};
int flags(const cmt_attn_train_args& a) { return 2 * (a.dn_pad > 0) + (a.dropout_p > 0.f); }

// forward over p.a.kv_splits key splits (+ the combine)
template <class A>
void launch_fwd(const cmt_attn_train_args& a, const AP& p, hipStream_t s) {
    const int splits = p.a.kv_splits;
    Pass<A>::fwd[flags(a)]<<<dim3(cdiv(a.Nq, 128), a.B * a.H, splits), 256, 0, s>>>(p);
    if (splits > 1) {
        const int64_t n = (int64_t)a.B * a.H * a.Nq * D;
        train_combine_kernel<<<(unsigned)cdiv64(n, 256), 256, 0, s>>>(p);
    }
}

// dQ over p.a.kv_splits key splits and dK / dV over ks query splits, after train_delta_kernel
template <class A>
int launch_bwd(const cmt_attn_train_args& a, const AP& p, int ks, hipStream_t s, const char* who) {
    const int qs = p.a.kv_splits;
    if (qs > 1)
        if (int rc = zero_grad(a.dQ, a.q_bs, a.q_hs, a.q_rs, a.B, a.H, a.Nq, s, who)) return rc;
    if (ks > 1) {
        if (int rc = zero_grad(a.dK, a.k_bs, a.k_hs, a.k_rs, a.B, a.H, a.Nk, s, who)) return rc;
        if (int rc = zero_grad(a.dV, a.v_bs, a.v_hs, a.v_rs, a.B, a.H, a.Nk, s, who)) return rc;
    }
    Pass<A>::dq[flags(a)]<<<dim3(cdiv(a.Nq, 128), a.B * a.H, qs), 256, 0, s>>>(p);
    Pass<A>::dkv[flags(a)]<<<dim3(cdiv(a.Nk, 128), a.B * a.H, ks), 256, 0, s>>>(p, cdiv(cdiv(a.Nq, KT), ks));
    return cmt_check_launch(who);
}

}  // namespace

extern "C" int64_t cmt_attn_train_workspace_bytes(const cmt_attn_train_args* a) {
    if (!a) return 0;
    return fast_path(*a) ? fast_ws(*a).total : split_ws_bytes(*a);
}

extern "C" int cmt_attn_train_fwd(const cmt_attn_train_args* ap, void* stream) {
    CMT_REQUIRE(ap != nullptr, "cmt_attn_train_fwd: null args");
    if (int rc = check_args(*ap, "cmt_attn_train_fwd")) return rc;
    const int splits = train_splits(*ap);
    // the long-key f16 path always writes its f16 copies into the workspace (also at one split)
    if ((splits > 1 || fast_path(*ap)) &&
        (ap->workspace == nullptr || ap->workspace_bytes < cmt_attn_train_workspace_bytes(ap)))
        return cmt_fail(CMT_EWORKSPACE, "cmt_attn_train_fwd: workspace too small");
    AP p = make_ap(*ap, splits);
    hipStream_t s = (hipStream_t)stream;
    if (fast_path(*ap)) {
        // f16 head-split operands (+ the keys' per-64-row max |k|^2), then the inference core with
        // the row statistic (attention.hip; output rounded to f16 like the flash core's)
        const cmt_attn_train_args& a = *ap;
        const FastWs w = fast_ws(a);
        char* base = (char*)a.workspace;
        f16_t* q16 = (f16_t*)(base + w.q16);
        f16_t* k16 = (f16_t*)(base + w.k16);
        f16_t* v16 = (f16_t*)(base + w.v16);
        float* kmax = (float*)(base + w.kmax);
        to16(a.Q, a.q_bs, a.q_hs, a.q_rs, a.B, a.H, a.Nq, q16, nullptr, s);
        to16(a.K, a.k_bs, a.k_hs, a.k_rs, a.B, a.H, a.Nk, k16, kmax, s);
        to16(a.V, a.v_bs, a.v_hs, a.v_rs, a.B, a.H, a.Nk, v16, nullptr, s);
        if (int rc = cmt_check_launch("cmt_attn_train_fwd (f16 copies)")) return rc;
        cmt_attn_args g = {};
        g.B = a.B; g.H = a.H; g.Nq = a.Nq; g.Nk = a.Nk; g.dtype = CMT_F16;
        g.Q = q16; g.q_bstride = (int64_t)a.H * a.Nq * D; g.q_hstride = (int64_t)a.Nq * D; g.q_rstride = D;
        g.K = k16; g.k_bstride = (int64_t)a.H * a.Nk * D; g.k_hstride = (int64_t)a.Nk * D; g.k_rstride = D;
        g.V = v16; g.v_bstride = g.k_bstride; g.v_hstride = g.k_hstride; g.v_rstride = D;
        g.O = a.O; g.o_bstride = a.o_bs; g.o_rstride = a.o_rs; g.o_dtype = CMT_F32;
        g.scale = a.scale;
        g.flags = CMT_ATTN_ROUND_OUTPUT;
        g.kv_splits = fwd_splits(a);
        g.workspace = base + w.attn;
        g.workspace_bytes = w.total - w.attn;
        g.kmax2 = kmax; g.kmax_ld = a.H; g.kmax_plane0 = 0; g.kmax_rows = 64;
        return cmt_attn_fwd_lse(g, a.LSE, s);
    }
    if (ap->fp16_inputs) launch_fwd<F16>(*ap, p, s);
    else launch_fwd<F32>(*ap, p, s);
    return cmt_check_launch("cmt_attn_train_fwd");
}

extern "C" int cmt_attn_train_bwd(const cmt_attn_train_args* ap, void* stream) {
    CMT_REQUIRE(ap != nullptr, "cmt_attn_train_bwd: null args");
    if (int rc = check_args(*ap, "cmt_attn_train_bwd")) return rc;
    CMT_REQUIRE(ap->dO && ap->dQ && ap->dK && ap->dV && ap->delta, "cmt_attn_train_bwd: null gradient pointer");
    const cmt_attn_train_args& a = *ap;
    const int ntiles = cdiv(a.Nk, KT), nqt = cdiv(a.Nq, KT);
    // dQ key splits: one round at the kernel's 3 waves per SIMD (3 four-wave workgroups per CU:
    // 768); the power-of-two split ran 1.5 rounds at the coop self-attention shape (r6f: bwd
    // 377 -> 303 us with the dK / dV split below)
    const int qs = max(1, min(ntiles / 2, 768 / (cdiv(a.Nq, 128) * a.B * a.H)));
    AP p = make_ap(a, qs);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)a.B * a.H * a.Nq;
    train_delta_kernel<<<(unsigned)cdiv64(rows, 4), 256, 0, s>>>(p);
    if (fast_path(a) && a.workspace != nullptr && a.workspace_bytes >= fast_ws(a).total) {
        const FastWs w = fast_ws(a);
        char* base = (char*)a.workspace;
        f16_t* q16 = (f16_t*)(base + w.q16);
        f16_t* k16 = (f16_t*)(base + w.k16);
        f16_t* v16 = (f16_t*)(base + w.v16);
        f16_t* d16 = (f16_t*)(base + w.d16);
        to16(a.dO, a.o_bs, a.o_hs, a.o_rs, a.B, a.H, a.Nq, d16, nullptr, s);
        if (!a.ws_reuse) {   // ABI 25: else the forward's copies of Q / K / V are still in the workspace
            to16(a.Q, a.q_bs, a.q_hs, a.q_rs, a.B, a.H, a.Nq, q16, nullptr, s);
            to16(a.K, a.k_bs, a.k_hs, a.k_rs, a.B, a.H, a.Nk, k16, nullptr, s);
            to16(a.V, a.v_bs, a.v_hs, a.v_rs, a.B, a.H, a.Nk, v16, nullptr, s);
        }
        // dQ: key splits of 8-wave workgroups, about two per CU
        // (two 8-wave workgroups per CU: about 512 workgroups in one balanced round)
        const int nqb = cdiv(a.Nq, 256);
        const int ds = max(1, min(512 / (nqb * a.B * a.H), ntiles / 8));
        AP pq = make_ap(a, ds);
        if (ds > 1)
            if (int rc = zero_grad(a.dQ, a.q_bs, a.q_hs, a.q_rs, a.B, a.H, a.Nq, s, "cmt_attn_train_bwd")) return rc;
        const int nqp = cdiv(a.Nq, 64) * 64;
        train16_dkv2_kernel<<<dim3((unsigned)cdiv(a.Nk, 256), (unsigned)(a.B * a.H)), 512, 0, s>>>(p, q16, d16, k16,
                                                                                                   v16, nqp);
        train16_dq2_kernel<<<dim3((unsigned)nqb, (unsigned)(a.B * a.H), (unsigned)ds), 512, 0, s>>>(pq, q16, d16, k16,
                                                                                                    v16);
        return cmt_check_launch("cmt_attn_train_bwd");
    }
    // the f16 form takes no dK / dV query splits; f32: one round at the kernel's 2 waves per SIMD
    // (2 four-wave workgroups per CU: 512)
    if (a.fp16_inputs) return launch_bwd<F16>(a, p, 1, s, "cmt_attn_train_bwd");
    const int ks = max(1, min(nqt / 2, (int)(512 / ((int64_t)cdiv(a.Nk, 128) * a.B * a.H))));
    return launch_bwd<F32>(a, p, ks, s, "cmt_attn_train_bwd");
}

// ---------------------------------------------------------------------------
// The fp32 core on three bf16 MFMA passes (policy X3).  Grids and splits, chosen at the coop
// self-attention shape (B 2, H 8, Nq = Nk = 1 100, DN 200 / 20, p 0.1: 144 workgroups per split in
// every kernel, 18 tiles; kernel-trace averages, profiles/train_attn_x3.txt):
//   forward   key splits train_splits() as the exact-f32 entry point (+ train_combine_kernel, same
//             workspace layout): 4 splits; kernel + combine 36.1 + 9.5 us at 3, 32.4 + 11.5 at 4,
//             35.5 + 14.5 at 6
//   dQ        key splits min(tiles / 2, 432 / workgroups), f32 atomics into a zeroed dQ: 3 splits;
//             78.4 us at 2, 72.7 at 3, 92.1 at 5 (the exact-f32 rule's 768) -- the atomic
//             traffic grows with the splits and these kernels no longer hide it behind the MFMAs
//   dK / dV   query splits min(query tiles / 2, 288 / workgroups), f32 atomics into zeroed dK / dV:
//             2 splits; 115.2 us at 2, 120.3 at 3 (the exact-f32 rule's 512), 145.3 at 4; one split
//             (144 workgroups on 256 CUs) measured 175.6 us against 163.3 / 141.9 at 2 / 3 before the
//             transposed LDS reads
// ---------------------------------------------------------------------------
namespace {

int check_args_x3(const cmt_attn_train_args* ap, const char* who) {
    CMT_REQUIRE(ap != nullptr, std::string(who) + ": null args");
    if (int rc = check_args(*ap, who)) return rc;
    CMT_REQUIRE(ap->fp16_inputs == 0, std::string(who) + ": fp16_inputs is the flash fp16 core (cmt_attn_train_fwd / _bwd)");
    return 0;
}

}  // namespace

extern "C" int64_t cmt_attn_train_bf16x3_workspace_bytes(const cmt_attn_train_args* a) {
    return a ? split_ws_bytes(*a) : 0;
}

extern "C" int cmt_attn_train_fwd_bf16x3(const cmt_attn_train_args* ap, void* stream) {
    if (int rc = check_args_x3(ap, "cmt_attn_train_fwd_bf16x3")) return rc;
    const int splits = train_splits(*ap);
    if (splits > 1 && (ap->workspace == nullptr || ap->workspace_bytes < split_ws_bytes(*ap)))
        return cmt_fail(CMT_EWORKSPACE, "cmt_attn_train_fwd_bf16x3: workspace too small");
    launch_fwd<X3>(*ap, make_ap(*ap, splits), (hipStream_t)stream);
    return cmt_check_launch("cmt_attn_train_fwd_bf16x3");
}

extern "C" int cmt_attn_train_bwd_bf16x3(const cmt_attn_train_args* ap, void* stream) {
    if (int rc = check_args_x3(ap, "cmt_attn_train_bwd_bf16x3")) return rc;
    CMT_REQUIRE(ap->dO && ap->dQ && ap->dK && ap->dV && ap->delta, "cmt_attn_train_bwd_bf16x3: null gradient pointer");
    const cmt_attn_train_args& a = *ap;
    const int ntiles = cdiv(a.Nk, KT), nqt = cdiv(a.Nq, KT);
    const int qs = max(1, min(ntiles / 2, 432 / (cdiv(a.Nq, 128) * a.B * a.H)));              // dQ key splits
    const int ks = max(1, min(nqt / 2, (int)(288 / ((int64_t)cdiv(a.Nk, 128) * a.B * a.H))));   // dK / dV query splits
    AP p = make_ap(a, qs);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)a.B * a.H * a.Nq;
    train_delta_kernel<<<(unsigned)cdiv64(rows, 4), 256, 0, s>>>(p);
    return launch_bwd<X3>(a, p, ks, s, "cmt_attn_train_bwd_bf16x3");
}
