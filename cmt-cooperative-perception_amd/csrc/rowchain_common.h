// What the row-block chains of rowchain.hip (f16 / bf16) and rowchain_x3.hip
// (f16 pairs) share: the workgroup geometry, the parameter-block layout, the
// lane -> column map, the fp32 row / partials-tile accessors, the workgroups
// per row block (chain_parts: B2's grows by the split chain's head parts), the
// row LayerNorm and the swizzled operand-image address.
// Included by those two files only.
#pragma once
#include "cmt_common.h"

namespace {

constexpr int RB = 32;                    // query rows per workgroup
constexpr int CE = 256;                   // embed dims
constexpr int NWV = 8;                    // waves
constexpr int NTC = 64 * NWV;             // threads
constexpr int VPL = CE / NWV / 2;         // values per lane of a row (its 32-column tile, lane pair): 16

// The fp32 parameter blocks (cmt_hip.h cmt_chain_args.prm), offsets in floats.
constexpr int PRM_A = 1024, PRM_B = 3840;
namespace prm_a {                         // chain A
constexpr int bo = 0, ln_w = 256, ln_b = 512, bq = 768;
}
namespace prm_b {                         // chains B1 and B2 (one block)
constexpr int bo = 0, ln1_w = 256, ln1_b = 512, b1 = 768, b2 = 1792, ln2_w = 2048, ln2_b = 2304, post_w = 2560,
              post_b = 2816, bn = 3072;
}
static_assert(prm_a::bq + CE == PRM_A && prm_b::bn + 3 * CE == PRM_B, "parameter blocks end with bq / bn");

// workgroups per row block: chain A 1, B1 4 (FFN quarters), B2 3 (Q | K | V blocks; 1 on the last layer)
// plus, split chain B2 with head weights (cmt_chain_args.Wh), one per 256 columns of the task heads'
// first conv (head_parts = ceil(head_cols / 256))
__host__ __device__ constexpr int chain_parts(int kind, bool has_next, int head_parts = 0) {
    return kind == 0 ? 1 : kind == 1 ? 4 : (has_next ? 3 : 1) + head_parts;
}

// column of lane value r (4 consecutive per group r >> 2) in wave w's 32-column tile
__device__ __forceinline__ int chain_col(int wave, int lh, int r) {
    return wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
}

// 16-byte chunk ch of row lr of the operand image [32][256] 16-bit at `base` (a pointer into LDS, or
// a byte offset): the chunks of a row are XOR-swizzled by row & 15
template <typename P>
__device__ __forceinline__ P act_at(P base, int lr, int ch) { return base + lr * (CE * 2) + ((ch ^ (lr & 15)) << 4); }

// this lane's VPL fp32 values of `row` (columns chain_col) from a [rows][256] fp32 matrix
__device__ __forceinline__ void load_row(const float* M, int row, int wave, int lh, float (&v)[VPL]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 x = *(const f32x4*)(M + (int64_t)row * CE + wave * 32 + 8 * g + 4 * lh);
        v[4 * g] = x[0];
        v[4 * g + 1] = x[1];
        v[4 * g + 2] = x[2];
        v[4 * g + 3] = x[3];
    }
}

__device__ __forceinline__ void store_row(float* M, int row, int wave, int lh, const float (&v)[VPL]) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *(f32x4*)(M + (int64_t)row * CE + wave * 32 + 8 * g + 4 * lh) =
            f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
}

// The B1 -> B2 partials workspace is private to the chains, so it is kept in
// the lanes' own order: per (plane, row block, wave, 16-byte group j) one
// contiguous 1 KB slab, lane-major.  Every wave instruction then moves 1 KB
// of consecutive bytes (8 cache lines) instead of 32-byte pieces of 32 rows
// (32 lines), which is what bounded chain B2 (~9 us for one workgroup).
__device__ __forceinline__ void load_tile(const float* M, int rb, int wave, int lane, float (&v)[VPL]) {
    const float* p = M + (int64_t)rb * RB * CE + wave * (VPL * 64) + lane * 4;
#pragma unroll
    for (int j = 0; j < VPL / 4; ++j) {
        const f32x4 x = *(const f32x4*)(p + j * 256);
        v[4 * j] = x[0];
        v[4 * j + 1] = x[1];
        v[4 * j + 2] = x[2];
        v[4 * j + 3] = x[3];
    }
}

__device__ __forceinline__ void store_tile(float* M, int rb, int wave, int lane, const float (&v)[VPL]) {
    float* p = M + (int64_t)rb * RB * CE + wave * (VPL * 64) + lane * 4;
#pragma unroll
    for (int j = 0; j < VPL / 4; ++j)
        *(f32x4*)(p + j * 256) = f32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
}

// A thread's place in the workgroup and the row epilogues that need only that: the parameter
// block at LDS byte OFF_PRM and the 2 x NWV x RB fp32 reduction slots at OFF_RED (template
// parameters, so every LDS access keeps an immediate offset).
template <int OFF_PRM, int OFF_RED>
struct RowCtx {
    char* lds;
    int lane, wave, lr, lh;

    __device__ __forceinline__ int col(int r) const { return chain_col(wave, lh, r); }
    __device__ __forceinline__ const float* prm() const { return (const float*)(lds + OFF_PRM); }

    // sum over the row's 256 columns (this lane's 16, the lane pair, the 8 waves); slots alternate
    __device__ __forceinline__ float row_sum(float x, int slot) const {
        x = pair_sum(x);
        float* red = (float*)(lds + OFF_RED);
        if (lh == 0) red[(slot * NWV + wave) * RB + lr] = x;
        barrier_mem();
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) t += red[(slot * NWV + w) * RB + lr];
        return t;
    }

    // in-place LayerNorm (nn.LayerNorm: biased variance) with weight / bias at parameter offsets
    __device__ __forceinline__ void layernorm(float (&v)[VPL], int w_off, int b_off, float eps) const {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) s += v[i];
        const float mean = row_sum(s, 0) * (1.f / CE);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const float d = v[i] - mean;
            q += d * d;
        }
        const float rstd = rsqrtf(row_sum(q, 1) * (1.f / CE) + eps);
        const float* pw = prm() + w_off;
        const float* pb = prm() + b_off;
#pragma unroll
        for (int r = 0; r < VPL; ++r) {
            const int c = col(r);
            v[r] = (v[r] - mean) * rstd * pw[c] + pb[c];
        }
    }
};

}  // namespace
