/*
 * cmt_hip.h -- C ABI of the MI355X-native CMT / CMTCoop decoder-head hot path.
 *
 * Build: libcmt_hip.so (hipcc --offload-arch=gfx950), see
 * cmt-cooperative-perception_amd/csrc/Makefile.  Consumers: the registered
 * Python classes in cmt-cooperative-perception_amd/projects/mmdet3d_plugin
 * (ctypes, native.py) -- the drop-in for the reference's
 * projects/mmdet3d_plugin heads/transformer/attention/voxelization.
 *
 * Contract:
 *   - plain pointers + sizes; every pointer is a device pointer unless noted;
 *   - the caller (PyTorch) owns every buffer; nothing here allocates device
 *     memory -- scratch space is a caller-provided workspace whose size is
 *     returned by the matching *_workspace_bytes query;
 *   - stream-ordered and reentrant: every call takes the stream (a hipStream_t
 *     passed as void*), launches asynchronously on it, never synchronises and
 *     keeps no global mutable state (graph-capturable);
 *   - errors: every entry point returns 0 on success, a CMT_E* argument-check
 *     code, or the hipError_t of a failed launch; cmt_last_error() returns a
 *     thread-local message describing the last failure.
 *
 * Element type codes (dtype arguments).
 */
#ifndef CMT_HIP_H
#define CMT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMT_ABI_VERSION 25

/* CMT_F16P (ABI 12), "f16 pair": an fp32 operand split into two f16 halves,
 * x = hi + lo with hi = f16(x), lo = f16(x - hi).  Representation error:
 * |x - hi - lo| <= max(2^-22 |x|, 2^-25).  The relative 2^-22 (22 significant
 * bits) holds only while lo is itself a normal f16 number, i.e. for |x| >= ~2^-3;
 * below that lo is subnormal and the error is the absolute 2^-25 (the f16
 * subnormal half-step): ~2^-19 relative at |x| ~ 0.05, the scale of xavier
 * weights of a 256-wide layer, ~2^-16 at |x| ~ 0.005.  |x| must stay below
 * 65504.  A row of logical width C is stored as C hi values followed by C lo
 * values ([rows][2C] 16-bit words, leading dimensions in 16-bit elements).  A
 * GEMM whose A and W are both CMT_F16P computes A_hi W_hi + A_lo W_hi + A_hi W_lo
 * with fp32 accumulation (three f16 MFMA passes; the dropped A_lo W_lo term is
 * <= 2^-22 of a product): per product the error is the two operands'
 * representation errors above (tests/test_gpu_split.py::
 * test_gemm_split_small_weights holds the kernel to that bound on xavier-range
 * weights), at 3/16 of the f16 rate instead of the exact-f32 MFMA's 1/16.
 * Producers (LayerNorm, layout, geometry, GEMM epilogues, attention outputs)
 * write this format directly. */
enum cmt_dtype { CMT_F32 = 0, CMT_F16 = 1, CMT_BF16 = 2, CMT_F16P = 3 };

enum cmt_status {
    CMT_OK = 0,
    CMT_EINVAL = 1001,    /* bad argument (shape, alignment, dtype combination) */
    CMT_ENOTSUP = 1002,   /* unsupported configuration */
    CMT_EWORKSPACE = 1003 /* workspace too small */
};

int cmt_abi_version(void);
const char* cmt_last_error(void);

/* sizeof() of each argument struct as compiled into the library: a binding
 * that mirrors a struct (ctypes, cffi) asserts its own size against these
 * before the first call (native.py does; so does the INTEGRATION.md stub). */
int64_t cmt_gemm_args_size(void);
int64_t cmt_attn_args_size(void);
int64_t cmt_ln_args_size(void);
int64_t cmt_chain_args_size(void);
int64_t cmt_gemm_ex_args_size(void);
int64_t cmt_attn_train_args_size(void);
int64_t cmt_ln_train_args_size(void);
int64_t cmt_bn_args_size(void);
int64_t cmt_det_loss_args_size(void);
int64_t cmt_match_cost_args_size(void);
int64_t cmt_adamw_args_size(void);
int64_t cmt_lsap_args_size(void);

/* ------------------------------------------------------------------------
 * GEMM with fused prologue/epilogue (MFMA, gfx950).
 *   C[m, n] = act( sum_k Aeff[m, k] * W[n, k] + bias[n] ) + R[m, n]
 * Replaces the cuBLAS GEMMs of the reference:
 *   FlashMHA _in_projection_packed      models/utils/attention.py:21-27,130
 *   FlashMHA out_proj                   models/utils/attention.py:117,138
 *   nn.MultiheadAttention in/out proj   (mmcv MultiheadAttention, attn_cfgs[0])
 *   mmcv FFN fc1/fc2                    (ffn_cfgs, e.g. configs/.../cmt_lidar_voxel0075_cbgs.py:232-239)
 *   bev_embedding / rv_embedding MLPs   models/dense_heads/cmt_head.py:292-301
 *   shared_conv Conv2d 3x3 (+BN fold)   models/dense_heads/cmt_head.py:280-287  (a_mode = CONV3X3)
 *   SeparateTaskHead grouped Conv1d     models/dense_heads/cmt_head.py:136-159  (a_mode = CONV1D3, batch = groups)
 * Output columns n < a2_cols see a modified A (the positional-encoding add
 * `key = key + key_pos`, petr_transformer.py:296-299):
 *   a2_mode CMT_A2_ADD     Aeff = A + A2 (both fp32, added on load);
 *   a2_mode CMT_A2_SELECT  Aeff = A2 (same dtype/strides as A: the caller
 *                          already holds the sum, e.g. written by the LN that
 *                          produced A), so one launch serves Q|K (pos) and V.
 * Compute dtype = w_dtype: CMT_F32 (exact-f32 MFMA 32x32x2), CMT_F16 or
 * CMT_BF16 (MFMA 32x32x16, fp32 accumulate).  With A in the compute dtype the
 * tiles are staged by LDS-DMA (global_load_lds); fp32 A is converted on load.
 * R may be fp32 or the compute dtype (r_dtype).
 * Requirements: N % 64 == 0, K % 32 == 0 (K % 64 for compute-dtype A),
 * 16-byte aligned A/W rows, ldc/ldr multiples of 4.
 * ------------------------------------------------------------------------ */
/* CMT_A_CONV3X3_NCHW (ABI 14): the 3x3 / pad 1 conv straight from an fp32 NCHW map
 * A[b * a_bstride + c * (conv_h * conv_w) + pixel] (lda unused), K = 9 * conv_c tap-major
 * as CONV3X3, M = conv_h * conv_w per batch element; split (CMT_F16P) W (the
 * reference-numerics shared_conv: each input pixel is split into f16 hi / lo once per
 * workgroup and serves all nine taps from LDS; fp32 or CMT_F16P row C) or, since round 6,
 * f16 / bf16 W (one MFMA pass on pixels rounded to W's dtype; fp32 or W-dtype row C);
 * conv_c % 16 == 0, conv_w <= 180, N % 128 == 0.  Optional second output: with A2 (fp32 rows
 * A2[m * lda2 + n], the same for every batch element -- the weight-only BEV position
 * rows) it also writes out + A2 at C + c_split_stride (same layout as C): lowp(memory +
 * pos), the K-projection operand, without a separate GEMM. */
enum cmt_gemm_amode { CMT_A_ROWS = 0, CMT_A_CONV3X3 = 1, CMT_A_CONV1D3 = 2, CMT_A_CONV3X3_NCHW = 3 };
enum cmt_gemm_cmode { CMT_C_ROWS = 0, CMT_C_HEADSPLIT = 1 };
enum cmt_gemm_a2mode { CMT_A2_ADD = 0, CMT_A2_SELECT = 1 };

typedef struct cmt_gemm_args {
    int M, N, K;
    int batch;                 /* grid z; per-batch strides below (elements) */
    const void* A; int64_t lda; int64_t a_bstride; int a_dtype;
    const void* A2; int64_t lda2; int a2_cols; int a2_mode;
    int a_mode;                /* cmt_gemm_amode */
    int conv_h, conv_w, conv_c;/* CONV3X3: NHWC input [M/(h*w)][h][w][c], K = 9*c */
    int seg_len;               /* CONV1D3: rows form segments of seg_len (zero pad), K = 3*C */
    const void* W; int64_t ldw; int64_t w_bstride; int w_dtype;
    const float* bias; int64_t bias_bstride;
    const void* R; int64_t ldr; int64_t r_bstride; int r_dtype;
    void* C; int64_t ldc; int64_t c_bstride; int c_dtype;
    int c_mode;                /* cmt_gemm_cmode; HEADSPLIT: C[(b*(N/32)+n/32)*rows_per_batch + r][32]
                                  (a CMT_F16P C: [..][64], the 32 hi values then the 32 lo values) */
    int rows_per_batch;
    int relu;
    /* optional (HEADSPLIT with a 16-bit C only): plane_max2[(m/64)*(plane_max_cols/32) + n/32]
     * = max over the 64-row block's rows m of sum_{32 cols of head plane n/32} C[m,n]^2
     * (of the stored, rounded values), for n < plane_max_cols; every entry is written
     * (rows >= M count as 0).  Feeds cmt_attn_args.kmax2. */
    float* plane_max2; int plane_max_cols;
    /* optional split-K (ABI 13): k_splits >= 2 splits the logical K into k_splits equal
     * parts (K / k_splits % 64 == 0) run by separate workgroups; part s writes its partial
     * product to C + s * c_split_stride (fp32, row mode, batch 1, no relu), bias and R
     * are added by part 0 only, so the sum of the parts is the GEMM's output.  For the
     * decoder's 900-row GEMMs, whose tile grid alone covers a quarter of the CUs; the
     * LayerNorm after them sums the parts (cmt_ln_args.nparts).  0 or 1: no split. */
    int k_splits; int64_t c_split_stride;
    /* optional f16-operand range guard (ABI 18; the split (CMT_F16P) cmt_gemm kernels: the x3
     * tiles, CMT_A_CONV3X3_NCHW and the 128-wide split tile -- not cmt_kv_proj / cmt_gemm_ln,
     * whose operands are outputs of guarded kernels): when a pre-activation value -- or the second output of
     * CMT_A_CONV3X3_NCHW with A2 -- is non-finite or |x| >= 65520 (outside the f16-pair
     * format: a bad input element makes every output of its 3x3 neighbourhood NaN / inf, since
     * 0 x inf is NaN), the kernel ORs 1 into *range_flag.  Never cleared by the library: the
     * caller zeroes it and reads it after the stream (or a replayed graph) has run.  NULL: off. */
    int* range_flag;
} cmt_gemm_args;

int cmt_gemm(const cmt_gemm_args* args, void* stream);

/* cmt_kv_proj: the cross-attention K/V projection of ALL decoder layers in one
 * launch (kvproj.hip) -- FlashMHA's packed in_proj on the memory side
 * (attention.py:21-27, 126-138; key = key + key_pos at petr_transformer.py:
 * 296-299).  Same cmt_gemm_args contract as cmt_gemm restricted to: K = 256,
 * f16/bf16 A / W / C, row A, head-split C, no R / relu, batch 1, A2 (if any)
 * in select mode on exactly the first N/2 columns, N % (256 * parts) == 0,
 * optional plane_max2.  W is in the FRAGMENT-PACKED layout
 *   Wp[((p * 16 + ks) * 64 + lane) * 8 + e] = W[32 p + (lane & 31)][16 ks + 8 (lane >> 5) + e]
 * (torch: W.view(N/32, 32, 16, 2, 8).permute(0, 2, 3, 1, 4)), ldw unused.
 * c_bstride (16-bit elements, 0: (N/32) * rows_per_batch * 32) is the batch
 * stride of the head-split C, so one layer's K and V planes can be written into
 * a larger [B][planes][Nk][32] buffer (one launch per layer, C pointing at the
 * layer's first plane). */
int cmt_kv_proj(const cmt_gemm_args* args, void* stream);

/* cmt_mlp2_x3 (ABI 15): Linear(K, Hd) + ReLU + Linear(Hd, 256) in one launch at the
 * reference's fp32 numerics (mlp.hip) -- the camera position encoder rv_embedding
 * (cmt_head.py:297-301, applied at 433 on the frustum coordinates of _rv_pe and at
 * 464 on the query coordinates of _rv_query_embed).  Replaces the two cmt_gemm
 * calls (fc1 -> hidden pair rows in HBM -> fc2): the hidden activation never
 * leaves the registers.  Every product is the split-f16 three-pass product of
 * cmt_gemm (hi*hi + lo*hi + hi*lo, fp32 accumulation, fc1 in cmt_gemm's k order,
 * so the hidden values equal the two-GEMM path's bit for bit).
 *   A   CMT_F16P rows [M][2][K] (lda, a_bstride in 16-bit words), K % 16 == 0, K <= 192
 *   W1p / W2p  the fragment packs of the pair weights W1 [Hd][2][K] and W2 [256][2][Hd]
 *       (Hd % 32 == 0):
 *       W1p[(((hb * K/16 + ks) * 2 + pl) * 64 + lane) * 8 + j]
 *           = W1[32 hb + (lane & 31)][pl][16 ks + 8 (lane >> 5) + j]
 *       W2p[((((hb * 8 + ot) * 2 + s) * 2 + pl) * 64 + lane) * 8 + j]
 *           = W2[32 ot + (lane & 31)][pl][32 hb + 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)]
 *       (the second k order is the hidden accumulator's register order: fc1's
 *       output tile is fc2's operand without leaving the registers)
 *   b1 [Hd] (Hd <= 2048), b2 [256] fp32; out = fc2(relu(fc1(A) + b1)) + b2 (+ R)
 *   R   optional residual rows (CMT_F16P [.][2][256] or fp32), ldr / r_bstride
 *   C   CMT_F16P or fp32 rows, ldc / c_bstride (16-bit words for a pair C, else
 *       elements); batch = grid y. */
typedef struct cmt_mlp2_args {
    int M, K, Hd, N;           /* N must be 256 */
    int batch;
    const void* A; int64_t lda; int64_t a_bstride;
    const void* W1p; const float* b1;
    const void* W2p; const float* b2;
    const void* R; int64_t ldr; int64_t r_bstride; int r_dtype;
    void* C; int64_t ldc; int64_t c_bstride; int c_dtype;
    /* ABI 20, the camera memory rows in one launch (each optional, NULL = off; K == 192):
     * geo_i2l: A is not read but generated -- the _rv_pe frustum coordinates of
     *   cmt_rv_pe_coords (cmt_head.py:417-432, the same arithmetic and f16-pair split): row r of
     *   batch z is pixel r % (geo_h * geo_w) of view v = r / (geo_h * geo_w), V = M / (geo_h *
     *   geo_w) views per batch element, inverse matrix geo_i2l[(z * V + v) * 16], geo_D = K / 3
     *   depths up to geo_depth_max, geo_pc the point-cloud range;
     * rx: the residual R is read from the NCHW fp32 image features instead (the camera memory
     *   rows "(bs v) c h w -> bs (v h w) c", cmt_transformer.py:104-105): element n of row r is
     *   rx[((z * V + v) * 256 + n) * geo_h * geo_w + pixel]; it enters as its f16 pair (the
     *   rounding cmt_nchw_to_rows applies), those pair rows are written to C2 (ldc2 / c2_bstride
     *   in 16-bit words: the memory rows themselves), and a value the pair format cannot carry
     *   ORs 1 into *range_flag (optional) as cmt_nchw_to_rows_ex does. */
    const float* geo_i2l; int geo_h, geo_w, geo_D; float geo_pad_h, geo_pad_w, geo_depth_max;
    float geo_pc[6];
    const float* rx; void* C2; int64_t ldc2; int64_t c2_bstride; int* range_flag;
} cmt_mlp2_args;

int cmt_mlp2_x3(const cmt_mlp2_args* args, void* stream);
int64_t cmt_mlp2_args_size(void);

/* cmt_mlp2_affine (additive to ABI 25): rv_embedding over the _rv_pe frustum coordinates
 * without the fc1 GEMM.  The normalised coordinate of view b, pixel (u, v), depth d, axis c is
 *   (d (M_b[c][0] u + M_b[c][1] v + M_b[c][2]) + M_b[c][3] - lo_c) / span_c      (M_b = geo_i2l),
 * affine in (u, v), and nothing nonlinear stands before rv_embedding[0]; so hidden unit j is
 *   relu(alpha_bj u + beta_bj v + gamma_bj),   evaluated as fmaf(alpha, u, fmaf(beta, v, gamma)),
 *   alpha_bj = sum_c T1[j][c] M_b[c][0],   beta_bj = sum_c T1[j][c] M_b[c][1],
 *   gamma_bj = sum_c (T1[j][c] M_b[c][2] + T0[j][c] (M_b[c][3] - lo_c)) + b0[j]
 * with the weight-only tables T1[j][c] = sum_d W0[j][3 d + c] depth_d / span_c and
 * T0[j][c] = sum_d W0[j][3 d + c] / span_c.  The kernel contracts them with the camera matrices
 * per workgroup in float64 and rounds the coefficients to fp32.
 *   tab  float64 [Hd][8]: T1[j][0..2], T0[j][0..2], b0[j], 0     (16-byte aligned)
 *   m    as for cmt_mlp2_x3: Hd (% 32 == 0, at most 1024; CMT_ENOTSUP beyond), W2p, b2, C and
 *        the row strides; geo_i2l, geo_h, geo_w, geo_pad_h, geo_pad_w and geo_pc[0..2] (lo) give
 *        the rows' views and pixels (M % (geo_h * geo_w) == 0, and geo_h * geo_w % 32 == 0 --
 *        CMT_ENOTSUP otherwise: a wave's 32 rows lie in one view); rx and C2 together select the
 *        fused camera-row epilogue of cmt_mlp2_x3, else C = out (+ R) rows.  A, K, W1p, b1,
 *        geo_D and geo_depth_max are not read (the depths and spans are in the tables). */
typedef struct cmt_mlp2_affine_args {
    cmt_mlp2_args m;
    const double* tab;
} cmt_mlp2_affine_args;

int cmt_mlp2_affine(const cmt_mlp2_affine_args* args, void* stream);
int64_t cmt_mlp2_affine_args_size(void);

/* ------------------------------------------------------------------------
 * Multi-head attention core, head_dim = 32 (flash-style, online softmax,
 * f16/bf16 MFMA with fp32 accumulate, or exact-f32 MFMA for dtype CMT_F32;
 * no mask).
 * Replaces flash_attn_unpadded_kvpacked_func (flash-attn 0.2.2) called at
 *   models/utils/attention.py:70-74 (FlashAttention.forward 46-92, fp16 core)
 * and the softmax(QK^T/sqrt(d))V core of nn.MultiheadAttention used by the
 * self-attention (mmcv MultiheadAttention, attn_cfgs[0]).
 * Element (b, h, row, d) of Q/K/V is at X[b*x_bstride + h*x_hstride + row*x_rstride + d]
 * (head-split layout: rstride = 32; token-major [B,S,H*32]: rstride = H*32;
 * sequence-first [S,B,H*32]: rstride = B*H*32).  Row strides must keep
 * 16-byte alignment (multiples of 8 elements).
 * Output O (o_dtype: fp32, or f16/bf16/f16-pair when it only feeds the
 * out-projection GEMM) has the heads concatenated per row (normalised).
 * dtype CMT_F16P (ABI 13, the reference-numerics self-attention): Q/K/V rows
 * are f16 pairs of 64 16-bit elements -- the 32 hi values, then the 32 lo
 * values (cmt_gemm's head-split pair C: rstride = 64) -- every product runs
 * as three f16 MFMAs (~2^-21 relative, fp32 softmax); strides count 16-bit
 * elements; no kv_splits, kmax2 or output rounding.
 * Nk is split into kv_splits chunks processed by separate workgroups and
 * merged by a combine pass (workspace: cmt_attn_workspace_bytes).
 * ------------------------------------------------------------------------ */
/* flags: CMT_ATTN_ROUND_OUTPUT  round O to dtype (flash-attn returns fp16)
 *        CMT_ATTN_FOLD_SCALE    the kernel may fold scale*log2(e) into Q when
 *                               it loads Q (one extra rounding of Q in the
 *                               compute dtype; used by the f16/bf16 policies,
 *                               not by the reference-numerics policy)
 *        CMT_ATTN_FORCE_PINGPONG, CMT_ATTN_FORCE_PIPELINED   reserved, ignored
 *                               (ABI 17 selected a software-pipelined variant
 *                               with the second; it measured slower and was
 *                               removed in round 5)
 *        CMT_ATTN_UNSCALED_Q       f16 long-key core without the fold
 *                               permission: Q enters the QK^T MFMAs unscaled
 *                               and the scores are scaled in fp32 (flash-attn's
 *                               order) instead of Q * scale as hi + lo
 *        CMT_ATTN_KEEP_PARTIALS (ABI 19) a split launch (cmt_attn_splits() > 1) skips its
 *                               combine pass and does not write O: the split partials stay in
 *                               the workspace for cmt_chain's chain B1 (cmt_chain_args.xpart) */
enum { CMT_ATTN_ROUND_OUTPUT = 1, CMT_ATTN_FOLD_SCALE = 2, CMT_ATTN_FORCE_PINGPONG = 256,
       CMT_ATTN_FORCE_PIPELINED = 512, CMT_ATTN_UNSCALED_Q = 1024, CMT_ATTN_KEEP_PARTIALS = 2048 };

typedef struct cmt_attn_args {
    int B, H, Nq, Nk;
    int dtype;                 /* CMT_F32, CMT_F16, CMT_BF16 or CMT_F16P (Q, K, V) */
    const void* Q; int64_t q_bstride, q_hstride, q_rstride;
    const void* K; int64_t k_bstride, k_hstride, k_rstride;
    const void* V; int64_t v_bstride, v_hstride, v_rstride;
    void* O; int64_t o_bstride, o_rstride;   /* O[b*o_bstride + q*o_rstride + h*32 + d] */
    int o_dtype;               /* CMT_F32 / CMT_F16 / CMT_BF16 / CMT_F16P (pair rows [hi H*32 | lo H*32]) */
    float scale;               /* softmax scale, usually 1/sqrt(32) */
    int kv_splits;             /* 0 = choose automatically */
    int flags;                 /* CMT_ATTN_ROUND_OUTPUT | CMT_ATTN_FOLD_SCALE */
    void* workspace; int64_t workspace_bytes;
    /* optional (NULL = off): max squared key-row norms written by the K
     * projection GEMM (cmt_gemm_args.plane_max2): entry [e][kmax_ld] covers key
     * rows e*kmax_rows .. +kmax_rows-1 of the batch-major K rows (b*Nk + row),
     * head h reads column kmax_plane0 + h.  With bf16 the long-key kernel then
     * fixes each query's softmax offset at the Cauchy-Schwarz bound |q|*max|k|
     * (no running max) when that bound is <= 60 in exp2 units. */
    const float* kmax2; int kmax_ld; int kmax_plane0; int kmax_rows;
} cmt_attn_args;

int64_t cmt_attn_workspace_bytes(const cmt_attn_args* args);
int cmt_attn_fwd(const cmt_attn_args* args, void* stream);
/* ABI 19: the key-split count a cmt_attn_fwd launch with these arguments uses (1 = no partials) */
int cmt_attn_splits(const cmt_attn_args* args);

/* ------------------------------------------------------------------------
 * LayerNorm over the last dim C (C % 64 == 0, C <= 1024), eps given.
 *   y = LN(x) * w + b   (nn.LayerNorm; mmcv build_norm_layer LN, eps 1e-5)
 * flags: CMT_LN_NAN_TO_NUM  apply torch.nan_to_num to y (cmt_head.py:499)
 *        CMT_LN_MAX_INTO    y = max(y, Y_old) (coop max-fusion, cmt_head_coop.py:388-389)
 * If W2/B2/Y2 are non-null a second LN is applied to the first LN's output
 * (the decoder post_norm of each layer output, petr_transformer.py:364-368)
 * and written to Y2 with its own flags2.
 * Pointer arguments named *_range6, *3 (voxel geometry) and head_out are HOST
 * arrays (read at launch); all other pointers are device pointers.
 * ------------------------------------------------------------------------ */
enum { CMT_LN_NAN_TO_NUM = 1, CMT_LN_MAX_INTO = 2 };
int cmt_layernorm(const float* X, int64_t ldx, int rows, int C,
                  const float* W, const float* Bv, float eps, float* Y, int64_t ldy, int flags,
                  const float* W2, const float* B2, float* Y2, int64_t ldy2, int flags2,
                  void* stream);

/* cmt_layernorm_ex: cmt_layernorm plus the next GEMMs' operands in the
 * compute dtype (lowp_dtype), written from the same registers:
 *   Yl[row] = lowp(y)            (e.g. the FFN / V-projection input)
 *   Yp[row] = lowp(y + P[row])   (query + query_pos, petr_transformer.py:296-297)
 * Y may be NULL when only the compute-dtype copies are needed. */
typedef struct cmt_ln_args {
    const float* X; int64_t ldx; int rows; int C;
    const float* W; const float* B; float eps;
    float* Y; int64_t ldy; int flags;
    const float* W2; const float* B2; float* Y2; int64_t ldy2; int flags2;
    int lowp_dtype;
    void* Yl; int64_t ldyl;
    void* Yp; int64_t ldyp; const float* P; int64_t ldp;
    /* ABI 13: the LayerNorm input is the sum of nparts (>= 1; 0 = 1) row blocks
     * X + p * part_stride -- the partial products of a split-K cmt_gemm */
    int nparts; int64_t part_stride;
} cmt_ln_args;
int cmt_layernorm_ex(const cmt_ln_args* args, void* stream);

/* cmt_gemm_ln: cmt_gemm followed by cmt_layernorm_ex on its output rows, in
 * one launch (the post-norm "x = LN(x + sublayer(x))" of
 * petr_transformer.py:374-487 for the attention out-projections and FFN fc2):
 * t = A W^T + bias + R is never written; ln->X is ignored and every LN output
 * of ln (Y, Yl, Yp, Y2) is produced.  Needs N == ln->C == 256, compute-dtype
 * A/W, row mode, batch 1.  ABI 14: A and W both CMT_F16P (the reference-numerics
 * out-projections + norms[0] / norms[1]: three f16 passes, fp32 R, pair Yl / Yp). */
int cmt_gemm_ln(const cmt_gemm_args* gemm, const cmt_ln_args* ln, void* stream);

/* ------------------------------------------------------------------------
 * Row-block chains of the decoder layer's query side (rowchain.hip): each
 * workgroup owns 32 complete query rows (C = 256) and runs the layer's GEMMs
 * back to back with their operands in LDS and the post-norm epilogues fused
 * (petr_transformer.py:374-487; mmcv FFN / LN).  Replaces, per layer, the
 * cuBLAS out_proj / in_proj / FFN GEMMs and the three LayerNorms around the
 * two attention cores (attention.py:117, mmcv MultiheadAttention, mmcv FFN).
 *   kind 0 (chain A, after self-attention; 1 workgroup per 32 rows):
 *     Y = norms[0](X Wo^T + bo + R);  Q = lowp(Y + P) Wq^T + bq  (head split [B][8][Nq][32])
 *   kind 1 (chain B1, after cross-attention; 4 workgroups per 32 rows, g = FFN quarter):
 *     o = norms[1](X Wo^T + bo + R);  h_g = relu(lowp(o) W1[256g:256g+256]^T + b1[...]);
 *     WS[g] = lowp(h_g) W2[:, 256g:256g+256]^T  (+ b2 + o for g = 0)     fp32 partials
 *   kind 2 (chain B2; 3 workgroups per 32 rows with Wn, else 1):
 *     Y = norms[2](WS[0] + WS[1] + WS[2] + WS[3])   (the next layer's query)
 *     OUT = post_norm(Y) (+ CMT_LN_NAN_TO_NUM / CMT_LN_MAX_INTO per out_flags)
 *     if Wn: Q = [lowp(Y + P) | lowp(Y + P) | lowp(Y)] Wn^T + bn  (next layer's
 *            self-attn in_proj, head split [B][24][Nq][32])
 *     if Wh (CMT_F16P only): H1 = pairs(OUT) Wh^T, ceil(head_cols / 256) more workgroups per 32 rows
 * prm: packed fp32 parameter block, layout (floats)
 *   A (1024): bo | norms[0].weight | norms[0].bias | bq
 *   B (3840, the same block for B1 and B2): bo | norms[1].w | norms[1].b | b1 (1024) | b2 |
 *             norms[2].w | norms[2].b | post_norm.w | post_norm.b | bn (768, zeros without Wn)
 * WS: caller workspace of cmt_chain_ws_bytes(rows) bytes = 4 * ceil(rows/32) * 32 * 256
 *     fp32 (B1 writes whole 32-row tiles, B2 reads them; private tile order).
 * One eps for every LayerNorm of the layer.  Weights / X / Q in the compute
 * dtype (f16 / bf16), residuals and outputs fp32; every buffer 16-byte aligned.
 * ------------------------------------------------------------------------ */
typedef struct cmt_chain_args {
    int kind;                  /* 0 = chain A, 1 = chain B1, 2 = chain B2 */
    int rows, Nq;              /* rows = B * Nq */
    int dtype;                 /* CMT_F16 / CMT_BF16 */
    float eps;
    const void* X;             /* A, B1: attention output [rows][256] */
    const float* R;            /* A, B1: residual [rows][256] fp32 (NULL = zeros) */
    const float* P;            /* query_pos [rows][256] fp32 (A; B2 with Wn) */
    const float* prm;          /* packed parameter block */
    const void* Wo;            /* A, B1: out_proj.weight [256][256] */
    const void* W1;            /* A: cross-attn in_proj_weight[:256], FRAGMENT-MAJOR (the Wn layout, g = 0);
                                  B1: fc1.weight [1024][256] row-major */
    const void* W2;            /* B1: fc2.weight [256][1024] as its 4 K blocks [256][256g..256g+256),
                                  each FRAGMENT-MAJOR (the Wn layout, g = K block) */
    const void* Wn;            /* B2: next layer's self-attn in_proj_weight [768][256], FRAGMENT-MAJOR:
                                  element W[256g + 64w + 32nt + r][32kc + 16ks + 8h + e] at
                                  ((((((g*4 + w)*8 + kc)*2 + ks)*2 + nt)*2 + h)*32 + r)*8 + e
                                  (NULL: last layer) */
    float* Y;                  /* A: norms[0] output; B2: norms[2] output; [rows][256] fp32 */
    float* OUT; int out_flags; /* B2: layer output [rows][256] fp32 */
    void* Q;                   /* head-split projection output (A; B2 with Wn) */
    float* WS;                 /* B1 / B2: partials workspace, 4 * ceil(rows/32) * 32 * 256 fp32 (private order) */
    void* OUT16;               /* B2 (optional): the layer output again in dtype (the task-head GEMM operand) */
    int wo_frag;               /* A: 1 = Wo is FRAGMENT-MAJOR (the Wn layout, g = 0) and streams into registers
                                  with W1 (no LDS weight ring); 0 = row-major Wo through the ring (ABI 10) */
    /* ABI 19, B1 with dtype CMT_F16P (optional, NULL = off): the cross-attention output as the split
     * partials a cmt_attn_fwd launch with CMT_ATTN_KEEP_PARTIALS left in its workspace (xpart = that
     * workspace; xsplits = cmt_attn_splits() of the launch, must be 8; B = rows / Nq, 8 heads).
     * Each workgroup combines its 32 rows itself (attn_combine_kernel's arithmetic, rounded to f16
     * when xround, as CMT_ATTN_ROUND_OUTPUT does) and X is not read. */
    const float* xpart; int xsplits; int xround;
    /* B2 with dtype CMT_F16P (optional, NULL = off; additive to ABI 25, cmt_chain_args_size tells a
     * stale mirror): the task heads' first grouped conv of this layer at final_kernel = 1, a per-row
     * linear map without bias.  Wh = its pair weight [head_cols][256], zero-padded to a multiple of
     * 256 rows and packed FRAGMENT-MAJOR like Wn (hi pack, then lo pack); H1 = fp32 [rows][head_cols]
     * = pairs(OUT) Wh^T, the product cmt_gemm gives on OUT16 with the same weight, bit for bit.
     * ceil(head_cols / 256) more workgroups per 32 rows compute it; OUT16 is then not needed.
     * head_cols % 64 == 0, 0 < head_cols <= 1024; not with CMT_LN_MAX_INTO (the fused maximum is
     * only complete after the last agent). */
    const void* Wh; float* H1; int head_cols;
} cmt_chain_args;
int cmt_chain(const cmt_chain_args* args, void* stream);
/* bytes of the B1 -> B2 partials workspace WS for `rows` query rows */
int64_t cmt_chain_ws_bytes(int rows);

/* cmt_add_cast: Yl = lowp(X), Yp = lowp(X + P) over rows x C (either output
 * may be NULL; X == NULL reads zeros, the zero target of cmt_transformer.py:114)
 * -- the decoder's first-layer operands from the initial target. */
int cmt_add_cast(const float* X, const float* P, int rows, int C, int lowp_dtype, void* Yl, void* Yp,
                 void* stream);

/* ------------------------------------------------------------------------
 * Coordinate encodings.
 * cmt_pos2embed: cmt_head.py:40-50.  pos [n, pos_stride] (x, y in the first two
 *   fp32 lanes), out [n, 2F] of odtype (F = num_pos_feats, F % 8 == 0: the y and
 *   the x half are each written in groups of 8 outputs; row stride ldo, ldo % 8
 *   == 0); mode 1 applies sigmoid(inverse_sigmoid(p)) first (query_embed,
 *   cmt_head.py:470).
 *   If pos == NULL the BEV grid centres (coords_bev, cmt_head.py:324-337) of a
 *   grid_h x grid_w map are generated in place of the input.
 * cmt_rv_pe_coords: _rv_pe geometry (cmt_head.py:417-432): out [BV*h*w, 3*D] (odtype)
 *   normalised lidar coordinates of D depth samples per image token; i2l is a
 *   [BV,4,4] fp32 device array of inv(lidar2img) (fp64 host inverse).
 * cmt_rv_query_coords: _rv_query_embed geometry (cmt_head.py:446-463):
 *   ref [B,Nq,3] (raw reference points; clamped + sigmoid(inverse_sigmoid)),
 *   l2i / i2l [B,V,4,4] fp32 -> out [B,V,Nq,3*D], mask [B,V,Nq] fp32 {0,1}.
 * cmt_masked_view_sum: (rv * mask).sum(dim=1) (cmt_head.py:466) added into Y:
 *   Y[b,q,:] += sum_v X[b,v,q,:] * mask[b,v,q].
 * cmt_rv_query_coords_ex (ABI 11): cmt_rv_query_coords with out in odtype
 *   (f16/bf16 rounded RNE: the operand of the rv_embedding GEMM without a cast pass).
 * cmt_masked_view_sum_ex (ABI 11): Y[b,q,:] = base[q,:] + sum_v ... (base [Nq,C]
 *   fp32, the BEV half of query_pos shared by every batch element; NULL: Y += ...),
 *   and optionally the decoder's first operands Yp = lowp(Y) = lowp(0 + query_pos)
 *   and Yl = lowp(0) (the zero target, cmt_transformer.py:114) in lowp_dtype.
 * ------------------------------------------------------------------------ */
int cmt_pos2embed(const float* pos, int64_t pos_stride, int n, int F, int mode,
                  int grid_h, int grid_w, void* out, int odtype, int64_t ldo, void* stream);
int cmt_rv_pe_coords(int BV, int h, int w, int D, float pad_h, float pad_w, float depth_max,
                     const float* i2l, const float* pc_range6, void* out, int odtype, void* stream);
int cmt_rv_query_coords(const float* ref, int B, int V, int Nq, int D, float pad_h, float pad_w,
                        const float* l2i, const float* i2l, const float* pc_range6,
                        float* out, float* mask, void* stream);
int cmt_masked_view_sum(const float* X, const float* mask, int B, int V, int Nq, int C,
                        float* Y, void* stream);
int cmt_rv_query_coords_ex(const float* ref, int B, int V, int Nq, int D, float pad_h, float pad_w,
                           const float* l2i, const float* i2l, const float* pc_range6,
                           void* out, int odtype, float* mask, void* stream);
int cmt_masked_view_sum_ex(const float* X, const float* mask, int B, int V, int Nq, int C,
                           const float* base, float* Y, void* Yl, void* Yp, int lowp_dtype, void* stream);

/* ------------------------------------------------------------------------
 * Layout / dtype plumbing.
 * cmt_nchw_to_rows: X [B, C, H*W] (optionally grouped as B = nb*nv images)
 *   -> rows: Y[(b_outer*rows_per_batch + row_offset + v*H*W + p)*ldy + c],
 *   i.e. rearrange "(bs v) c h w -> bs (v h w) c" (cmt_transformer.py:104-105),
 *   output dtype ydtype (CMT_F32/F16/BF16).
 * cmt_cast: elementwise dtype conversion of n elements.
 * ------------------------------------------------------------------------ */
int cmt_nchw_to_rows(const float* X, int nb, int nv, int C, int HW, void* Y, int ydtype,
                     int64_t ldy, int64_t rows_per_batch, int64_t row_offset, void* stream);
/* cmt_nchw_to_rows_ex (ABI 18): the same with the f16-operand range guard of
 * cmt_gemm_args.range_flag: for a CMT_F32 / CMT_F16 / CMT_F16P ydtype, an input element
 * that is non-finite or |x| >= 65520 ORs 1 into *range_flag (NULL: off; CMT_F32 with a flag:
 * rows a split-f16 consumer reads as pairs next, e.g. the training shared_conv). */
int cmt_nchw_to_rows_ex(const float* X, int nb, int nv, int C, int HW, void* Y, int ydtype,
                        int64_t ldy, int64_t rows_per_batch, int64_t row_offset, int* range_flag, void* stream);
int cmt_cast(const void* X, int xdtype, void* Y, int ydtype, int64_t n, void* stream);
/* cmt_split_rows (ABI 12): fp32 rows X[r * ldx + c] -> CMT_F16P rows Y [rows][2C]
 * (the split f16 GEMM operand of an fp32 tensor, e.g. the module-level API's inputs). */
int cmt_split_rows(const float* X, int64_t ldx, int64_t rows, int C, void* Y, void* stream);

/* ------------------------------------------------------------------------
 * SeparateTaskHead tail (cmt_head.py:136-203) + box epilogue (501-513).
 * H1 [L, B*Nq, nheads*hc] is the output of the first grouped conv (one GEMM
 * for all heads).  For every head: GroupLayerNorm1d over its hc channels
 * (eps 1e-6, biased var, cmt_head.py:56-66) -> ReLU -> grouped Conv1d
 * (kernel k along queries, zero pad) with weights W2 [L][out_total][k][hc]
 * packed per head, bias B2 [L][out_total].  Outputs are written to
 * OUT[L, B, Nq, out_total] (heads concatenated in order, widths head_out[]).
 * Columns listed by center_col/height_col receive the box epilogue:
 * sigmoid(x + inverse_sigmoid(ref)) * (max - min) + min.  H1 is only read;
 * the norm is applied to the LDS copy (one launch).
 * ------------------------------------------------------------------------ */
int cmt_task_head_tail(const float* H1, int L, int B, int Nq, int nheads, int hc,
                       const float* gln_w, const float* gln_b, const float* W2, const float* B2,
                       const int* head_out, int out_total, int k,
                       const float* ref, int center_col, int height_col, const float* pc_range6,
                       float* OUT, void* stream);

/* ------------------------------------------------------------------------
 * Point -> voxel scatter-mean (SPConvVoxelization + HardSimpleVFE).
 * Replaces spconv PointToVoxel at mmcv_custom/ops/voxel/spconv_voxelize.py:25-32,58-61
 * (called per sample at models/detectors/cmt.py:101-105) and mmdet3d
 * HardSimpleVFE.  Deterministic CPU semantics: voxels in first-appearance
 * order of their points, each keeps its first max_points points in input
 * order, at most max_voxels voxels, coordinates z,y,x.
 * A point is kept only if the fp32 quotient v = (p - range_min) / vsize
 * satisfies v >= 0 && v < (float)grid on all three axes, tested before any
 * conversion to int: NaN, +-inf and |v| >= 2^31 are dropped, -0.0 is cell 0.
 * points [N, F] fp32 (F >= nfeat_mean); outputs sized for max_voxels:
 *   voxels [max_voxels, max_points, F] (zero padded), coors [max_voxels, 3],
 *   num_points [max_voxels], means [max_voxels, nfeat_mean],
 *   num_voxels [1] (device int, M; -1 if the in-kernel scan gave up).
 * Three launches, no host synchronisation (graph-capturable).
 * Workspace (ABI 9): cmt_voxelize_workspace_bytes(N, .) bytes, filled once by
 * cmt_voxelize_workspace_init; every call leaves its hash table, look-back
 * words and ticket/error words all-ones again (the per-point and per-voxel
 * scratch arrays are rewritten by each call before it reads them), so one
 * workspace serves any number of calls with N up to its capacity (the
 * largest power of two >= 1024 whose layout fits workspace_bytes), on one
 * stream at a time.
 * ------------------------------------------------------------------------ */
int64_t cmt_voxelize_workspace_bytes(int N, int max_voxels);
int cmt_voxelize_workspace_init(void* workspace, int64_t workspace_bytes, void* stream);
int cmt_voxelize(const float* points, int N, int F, const float* voxel_size3,
                 const float* coors_range6, const int* grid3, int max_points, int max_voxels,
                 int nfeat_mean, float* voxels, int* coors, int* num_points, float* means,
                 int* num_voxels, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * NMS-free box decode.  Replaces
 * MultiTaskBBoxCoder.decode_single (core/bbox/coders/multi_task_bbox_coder.py:46-100)
 * + denormalize_bbox (core/bbox/util.py:37-68) for every sample b < B:
 *   logits [B][Nq*ncls] (last decoder layer, tasks' classes concatenated),
 *   bbox   [B][T*Nq][code] (center2, height1, dim3, rot2, vel2 per task block),
 *   class_task [ncls] = task index of each class label (device int32).
 * top-k (k = max_num) of sigmoid(logits), ties at the k-th value by lowest
 * index, score-descending; boxes denormalised (exp dims, atan2 yaw) to
 * code-1 values; kept if the center lies in post_center_range6 (HOST array)
 * and, when use_threshold, score > score_threshold.  Outputs are compacted in
 * rank order: out_boxes [B][max_num][code-1], out_scores/out_labels
 * [B][max_num], out_count [B] (device).  Nq*ncls <= 32768, max_num <= 1024.
 * ------------------------------------------------------------------------ */
int cmt_box_decode(const float* logits, int64_t logit_bstride, const float* bbox, int64_t bbox_bstride,
                   const int* class_task, int B, int Nq, int ncls, int code, int max_num,
                   const float* post_center_range6, float score_threshold, int use_threshold,
                   float* out_boxes, float* out_scores, int* out_labels, int* out_count, void* stream);

/* ========================================================================
 * TRAINING PATH (BASELINE configs[3] DDP training).
 * Exact-f32 kernels (the reference trains the head in fp32), used by the
 * torch.autograd Functions of projects/mmdet3d_plugin/models/utils/train_ops.py.
 * ======================================================================== */

/* cmt_gemm_f32_ex: C[z][m][n] = alpha * sum_k A(m,k) B(n,k) (+ bias[n]) + beta * C
 *   A(m,k) = A[z*a_bs + m*a_sm + k*a_sk],  B(n,k) = B[z*b_bs + n*b_sn + k*b_sk]
 * Any operand may be transposed (strides); k- or row-contiguous operands with
 * 16-byte alignment are staged by 16-byte loads.  ksplit > 1 splits K over
 * workgroups that add their partial sums into C with f32 atomics (beta = 1,
 * the caller initialises C).  Replaces the cuBLAS GEMMs of every nn.Linear
 * forward and backward (dX = dY W, dW = dY^T X) in the reference's training step. */
typedef struct cmt_gemm_ex_args {
    int M, N, K, batch;
    float alpha, beta;
    const float* A; int64_t a_sm, a_sk, a_bs;
    const float* B; int64_t b_sn, b_sk, b_bs;
    float* C; int64_t ldc, c_bs;
    const float* bias;         /* optional [N] per batch entry, at bias + z * bias_bs */
    int ksplit;
    int64_t bias_bs;           /* ABI 16: batch stride of bias (0: one bias for every z) */
    float* a_rowsum;           /* ABI 17, optional [batch][M], zero-initialised by the caller:
                                * += sum over this launch's k of A(m, k) in fp32 (cmt_gemm_bf16x3_ex
                                * only; a Linear's bias gradient from its weight-gradient GEMM) */
} cmt_gemm_ex_args;
int cmt_gemm_f32_ex(const cmt_gemm_ex_args* args, void* stream);
/* cmt_gemm_bf16x3_ex: the same contract, each fp32 operand split into a bf16
 * pair (hi + lo, RNE) and multiplied in three bf16 MFMA passes (lo*hi + hi*lo +
 * hi*hi, fp32 accumulate): ~2^-16 relative per product, fp32 exponent range --
 * the training step's Linear forward / dX / dW (the reference's fp32 cuBLAS
 * GEMMs, which torch 1.9.1 runs as TF32, ~2^-11, on Ampere by default). */
int cmt_gemm_bf16x3_ex(const cmt_gemm_ex_args* args, void* stream);
/* A Linear's backward in one call (ABI 23) on cmt_gemm_bf16x3_ex's arithmetic:
 * dX[M][K] = dY W (dX optional), dW[N][K] = dY^T X and dB[N] = the column sums of
 * dY (both optional; dB needs dW), with dY [M][N] and W [N][K] contiguous and X
 * [M][K] of row stride ldx.  dW and dB are overwritten: when the weight-gradient
 * reduction is split (ksplit > 1) or dB is asked for, they are zeroed on the
 * stream first and accumulated with f32 atomics.  Replaces, per call, the two
 * GEMM launches and the zero fill a caller of cmt_gemm_bf16x3_ex issues. */
int cmt_linear_bwd_bf16x3(const float* dY, const float* X, const float* W, float* dX, float* dW, float* dB,
                          int M, int K, int N, int64_t ldx, int ksplit, void* stream);
/* cmt_linear_bwd_bf16x3_ex (ABI 24): the same with flags.  CMT_LINEAR_BWD_ACCUMULATE: dW and dB
 * already hold a sum (a parameter's gradient) and the call ADDS to it -- no zero fill, the weight
 * gradient read-modify-written (unsplit) or f32-atomically added (split), the bias gradient added
 * atomically: the training step writes each Linear's weight gradient straight into the
 * parameter's .grad instead of returning it for autograd to add. */
#define CMT_LINEAR_BWD_ACCUMULATE 1
int cmt_linear_bwd_bf16x3_ex(const float* dY, const float* X, const float* W, float* dX, float* dW, float* dB,
                             int M, int K, int N, int64_t ldx, int ksplit, int flags, void* stream);

/* Attention forward with row statistics, and its backward (attn_train.hip),
 * exact f32, head_dim 32.  Replaces, in the training step, the fp32
 * self-attention core of nn.MultiheadAttention (with the DN mask of
 * cmt_head.py:386-398 and attn_drop) and the flash-attn 0.2.2 cross core
 * (attention.py:46-92; fp16_inputs = 1 rounds q, k, v, P and O to fp16 like
 * that core).  Element (b, h, row, d) of X at X[b*x_bs + h*x_hs + row*x_rs + d];
 * dQ / dK / dV use the strides of Q / K / V, dO those of O.
 * fwd writes O and LSE[b][h][q] = log2 sum_k exp2(c s_qk) (c = scale log2 e);
 * bwd reads Q, K, V, O, dO, LSE and writes dQ, dK, dV (delta: [B*H*Nq] scratch).
 * DN mask (dn_pad > 0): key k < dn_pad is hidden from query q if q >= dn_pad or
 * k / dn_group != q / dn_group.  dropout_p > 0: keep(q, k) from a counter hash
 * of (seed, b, h, q, k), identical in fwd and bwd (training only). */
typedef struct cmt_attn_train_args {
    int B, H, Nq, Nk;
    const float* Q; int64_t q_bs, q_hs, q_rs;
    const float* K; int64_t k_bs, k_hs, k_rs;
    const float* V; int64_t v_bs, v_hs, v_rs;
    float* O; int64_t o_bs, o_hs, o_rs;
    float* LSE;
    const float* dO; float* dQ; float* dK; float* dV; float* delta;
    float scale;
    int dn_pad, dn_group;
    int fp16_inputs;
    float dropout_p; uint32_t seed;
    int kv_splits;             /* fwd: 0 = automatic */
    void* workspace; int64_t workspace_bytes;
    const uint32_t* seed_dev;  /* ABI 22, optional: the dropout seed is seed + *seed_dev, read on the
                                * device (a graph-replayed step draws a fresh seed without re-capture) */
    int ws_reuse;              /* ABI 25, backward of the long-key path: nonzero = the workspace is the one
                                * the forward ran with on the same Q / K / V, so its f16 copies of them are
                                * reused and only dO is converted */
} cmt_attn_train_args;
/* Long-key fp16 path (ABI 15; fp16_inputs, no DN mask, no dropout, Nk >= 4096,
 * 128 < Nq <= 1152, heads contiguous in O (o_hs == 32), kv_splits 0 -- the
 * cross-attention of the training step): the forward runs cmt_attn_fwd's
 * bounded long-key core with the row statistic, the backward the dK/dV kernel
 * with the head's Q / dO resident in LDS and a K/V-streaming dQ kernel, all on
 * f16 copies of the operands held in the workspace.  cmt_attn_train_workspace_bytes
 * covers both directions; the forward returns CMT_EWORKSPACE on this path
 * with a smaller workspace, the backward runs the general kernels with less. */
int64_t cmt_attn_train_workspace_bytes(const cmt_attn_train_args* args);
int cmt_attn_train_fwd(const cmt_attn_train_args* args, void* stream);
int cmt_attn_train_bwd(const cmt_attn_train_args* args, void* stream);
/* cmt_attn_train_fwd_bf16x3 / _bwd_bf16x3: the same contract on the same struct
 * (fp16_inputs must be 0; ws_reuse is ignored) with the arithmetic of
 * cmt_gemm_bf16x3_ex in place of the 1/16-rate exact-f32 MFMA of the fp32 core:
 * every product (Q K^T, P V, dO^T P, dO V^T, K^T dS, Q^T dS) takes its fp32
 * operands split into a bf16 pair (hi + lo, RNE; Q, K, V, dO as they are staged,
 * P and dS from the fp32 accumulator) and runs as three bf16 MFMA passes
 * (lo*hi + hi*lo + hi*hi, fp32 accumulate): ~2^-16 relative per product, fp32
 * exponent range.  Scores, softmax statistics, LSE, delta, dS, the DN mask and
 * the dropout's kept set are those of the exact-f32 kernels; O is not rounded.
 * The workspace holds the forward's key-split partials only
 * (cmt_attn_train_bf16x3_workspace_bytes; CMT_EWORKSPACE with less). */
int64_t cmt_attn_train_bf16x3_workspace_bytes(const cmt_attn_train_args* args);
int cmt_attn_train_fwd_bf16x3(const cmt_attn_train_args* args, void* stream);
int cmt_attn_train_bwd_bf16x3(const cmt_attn_train_args* args, void* stream);

/* Row LayerNorm with saved statistics (C = 64 or 256): nn.LayerNorm
 * (mmcv LN, eps 1e-5) of the decoder and, with C = 64, eps 1e-6 and one weight
 * set per rows_per_wset rows, GroupLayerNorm1d (cmt_head.py:53-94) whose
 * custom backward (68-81) is the LayerNorm backward:
 *   dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w;
 *   dW[set] += sum dy xhat, dB[set] += sum dy (f32 atomics; zero them first). */
typedef struct cmt_ln_train_args {
    int rows, C;
    const float* X; int64_t ldx;
    const float* W; const float* B; float eps;
    int rows_per_wset;         /* 0 = one weight set */
    float* Y; int64_t ldy;     /* fwd output; bwd: dY reads ldy */
    float* mean; float* rstd;  /* [rows] saved by fwd, read by bwd */
    const float* dY; float* dX; int64_t lddx; int accumulate;
    float* dW; float* dB;
} cmt_ln_train_args;
int cmt_ln_train_fwd(const cmt_ln_train_args* args, void* stream);
int cmt_ln_train_bwd(const cmt_ln_train_args* args, void* stream);

/* BatchNorm2d in training mode (batch statistics over all NHWC rows, running
 * stats updated with momentum, unbiased running var) fused with ReLU: the
 * shared_conv ConvModule (cmt_head.py:280-287) after its 3x3 conv; and its
 * backward (dX, dW, dB).  workspace: cmt_bn_workspace_bytes(C). */
typedef struct cmt_bn_args {
    int rows, C;
    const float* X; float* Y;
    const float* W; const float* B; float eps; float momentum;
    float* running_mean; float* running_var;   /* optional */
    float* mean_save; float* rstd_save;        /* [C] */
    const float* dY; float* dX; float* dW; float* dB;
    void* workspace;
} cmt_bn_args;
int64_t cmt_bn_workspace_bytes(int C);
int cmt_bn_relu_train_fwd(const cmt_bn_args* args, void* stream);
int cmt_bn_relu_train_bwd(const cmt_bn_args* args, void* stream);

/* im2col of the 3x3 / pad 1 conv on NHWC rows (the weight-gradient operand of
 * shared_conv): out[(img*H+y)*W+x][tap*C + c], tap = 3*dy + dx. */
int cmt_im2col3x3(const float* X, int nimg, int H, int W, int C, float* out, void* stream);
/* The same weight gradient without the im2col matrix (ABI 21): dW[cout][tap*Cin + c]
 * = sum over the nimg*H*W rows r of dY[r][cout] * im2col(X)[r][tap*Cin + c], the
 * im2col elements gathered inside cmt_gemm_bf16x3_ex's kernel (its arithmetic);
 * ksplit > 1 adds into dW with f32 atomics (zero it first), 1 overwrites it.
 * Cin, Cout multiples of 4; X, dY 16-byte aligned. */
int cmt_conv3x3_wgrad_bf16x3(const float* X, const float* dY, float* dW, int nimg, int H, int W, int Cin,
                             int Cout, int ksplit, void* stream);

/* FocalLoss(use_sigmoid, gamma, alpha) + L1Loss of one task / decoder layer
 * (mmdet 2.28.2; cmt_head.py:702-720, 777-812): out[0] = cls loss, out[1] =
 * box loss; dlogits / dboxes (optional) receive d(loss)/d(input) * gscale.
 * labels == ncls is background.  One workgroup, fixed reduction order. */
typedef struct cmt_det_loss_args {
    int R, ncls;
    const float* logits; int64_t ld_logits;
    const int* labels; const float* label_w;
    int Rb;
    const float* boxes; int64_t ld_boxes;
    const float* targets; const float* box_w;  /* [Rb][10] */
    float gamma, alpha, cls_weight, box_weight, cls_avg, box_avg, gscale;
    float* out;                                 /* [2] */
    float* dlogits; float* dboxes;
} cmt_det_loss_args;
int cmt_det_loss(const cmt_det_loss_args* args, void* stream);

/* Hungarian cost matrix of HungarianAssigner3D (hungarian_assigner_3d.py:
 * 120-136): FocalLossCost (eps 1e-12) * cls_weight + BBox3DL1Cost over the
 * first 8 code-weighted box channels * reg_weight.  cost [Nq][ngt]. */
typedef struct cmt_match_cost_args {
    int Nq, ngt;
    const float* logits; int64_t ld_logits;
    const float* boxes; int64_t ld_boxes;
    const float* gt; const int* gt_labels;      /* gt [ngt][10] normalized */
    const float* code_w;                         /* [10] device */
    float gamma, alpha, cls_weight, reg_weight;
    float* cost;
} cmt_match_cost_args;
int cmt_match_cost(const cmt_match_cost_args* args, void* stream);

/* Batched rectangular linear sum assignment on the device: the
 * scipy.optimize.linear_sum_assignment call of HungarianAssigner3D
 * (hungarian_assigner_3d.py:139-147) for P independent cost matrices in one
 * call (a memset of status and two launches; additive to ABI 25).
 *   cost      one fp32 device buffer of cost_elems elements holding every
 *             matrix, [Nq][ngt] row-major as cmt_match_cost writes them.
 *   desc      [P][4] int64 in DEVICE memory: element offset into cost, Nq, ngt,
 *             row stride.  The host reads none of it: it only states P and the
 *             maxima max_nq / max_ngt that size the grid and the workspace.
 *   match_q   [P][ld_q] int32: match_q[p][j] = the query matched to GT j or -1
 *             (entries 0 .. ngt-1 are written, nothing else).
 *   match_g   [P][ld_g] int32, optional: match_g[p][q] = the GT matched to
 *             query q or -1 (entries 0 .. Nq-1): the gather form of the matching.
 *   status    [P] int32: 0 solved; 1 the matrix holds a NaN or an infinity (the
 *             ValueError of scipy); 2 a descriptor outside max_nq / max_ngt, the
 *             limits below or the cost buffer.  A problem with a non-zero status
 *             is not solved: all its matches are -1.
 * The smaller side is fully assigned (both ngt <= Nq and ngt > Nq work).
 * Method: the shortest augmenting path algorithm scipy uses (rectangular_lsap,
 * Crouse's Jonker-Volgenant variant), one wave per problem, dual variables and
 * path costs in float64 (fp32 costs are exact in it, scipy computes in it): on
 * a matrix whose optimum is unique the assignment equals scipy's.  An argmin
 * tie goes to the lowest column index, so a run is bitwise repeatable; on a
 * matrix with several optima the total cost equals scipy's, the assignment
 * need not.  Every loop is bounded by the shape (min(Nq, ngt) augmentations of
 * at most max(Nq, ngt) steps), and the finiteness check runs first.
 * Limits: max(max_nq, max_ngt) <= 2048, min(max_nq, max_ngt) <= 512, P <=
 * 65535 (CMT_ENOTSUP beyond); null pointers or P <= 0 give CMT_EINVAL before
 * any launch.  workspace: cmt_lsap_workspace_bytes(P, max_nq, max_ngt) bytes
 * (each matrix with its smaller side as rows). */
typedef struct cmt_lsap_args {
    int P, max_nq, max_ngt, reserved;
    const float* cost; int64_t cost_elems;
    const int64_t* desc;                         /* [P][4] device */
    int* match_q; int64_t ld_q;                  /* ld_q >= max_ngt */
    int* match_g; int64_t ld_g;                  /* optional; ld_g >= max_nq */
    int* status;                                 /* [P] */
    void* workspace; int64_t workspace_bytes;
} cmt_lsap_args;
int64_t cmt_lsap_workspace_bytes(int P, int max_nq, int max_ngt);
int cmt_lsap(const cmt_lsap_args* args, void* stream);

/* cmt_sumsq: *out += sum x^2 (zero *out first).  cmt_adamw_step:
 * torch.optim.AdamW over a flat buffer; if max_norm > 0 the gradient is scaled
 * by min(1, max_norm / (sqrt(*sumsq) + 1e-6)) (clip_grad_norm_, mmcv
 * OptimizerHook grad_clip). */
int cmt_sumsq(const float* x, int64_t n, float* out, void* stream);
typedef struct cmt_adamw_args {
    int64_t n; int step;
    float lr, beta1, beta2, eps, weight_decay, max_norm;
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    const float* sumsq;
} cmt_adamw_args;
int cmt_adamw_step(const cmt_adamw_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Sparse 3-D convolution (additive to ABI 25): the spconv half of mmdet3d's
 * SparseEncoder (pts_middle_encoder, models/detectors/cmt.py:78-86 of the
 * reference), inference only.  Rows are active sites: coors [n][4] int32
 * (b, z, y, x) and fp32 feature rows; every row count is an int32 in DEVICE
 * memory (a negative count reads as 0), buffers and launch grids are sized by a
 * host-side capacity, and no call synchronises with the host.
 *
 * Site index (cmt_sparse_index): for a grid (B, D, H, W) with B*D*H*W < 2^31
 * (CMT_EINVAL beyond) one bit per site, the number of set bits before each
 * 32-bit word, and a rank -> row table, so that "which row is site (b,z,y,x)"
 * is two loads and a popcount.  The table makes any row order valid (the
 * voxelizer emits first-appearance order); of several rows with equal
 * coordinates the lowest row index answers.  Rows outside the grid are ignored.
 * cmt_sparse_index_bytes(B, D, H, W, cap): ~ B*D*H*W / 4 + 4 cap bytes (21 MB for
 * one 41 x 1440 x 1440 sample); 0 for an invalid grid.
 *
 * Rulebooks.  K = kD*kH*kW taps, tap k = (kz*kH + ky)*kW + kx, nbr [rows][K]
 * int32, -1 where the neighbour is inactive or outside the grid.
 *   cmt_sparse_rulebook_subm (SubMConv3d: odd kernel3, stride 1, padding
 *     kernel3/2): nbr[m][k] = row of coors[m] + (kz,ky,kx) - padding3.  Output
 *     rows are the input rows.  Writes all n_cap rows (-1 beyond the count).
 *   cmt_sparse_rulebook_down (SparseConv3d, per-axis kernel3/stride3/padding3):
 *     output extent (n + 2p - k)/s + 1 per axis; an output site is active iff an
 *     active input lies in its window.  Writes out_coors [cap][4] in ascending
 *     (b, z, y, x) order -- independent of the input row order --, out_count (-1
 *     when more than cap outputs exist: nothing else is then valid), nbr
 *     [cap][K] with nbr[m][k] = row of out*stride3 - padding3 + (kz,ky,kx), and
 *     builds out_index (capacity cap) for the output set, so the next stage needs
 *     no cmt_sparse_index call.
 *
 * cmt_sparse_conv: Y[m] = act(scale * sum_k X[nbr[m][k]] W[k] + shift (+ R[m])),
 * fp32 rows in and out, Cin, Cout <= 128, K <= 27, for the first *count rows
 * (count <= cap).  nbr entries outside [0, n_in_cap) count as -1.  Arithmetic:
 * each operand split hi = bf16(x), lo = bf16(x - hi), products lo*hi + hi*lo +
 * hi*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation in fixed tap order
 * (no atomics: bit-reproducible; fp32 exponent range, ~2^-16 relative per
 * product).  Wp is the packed weight image of cmt_sparse_pack_bytes(K, Cin, Cout)
 * bytes: bf16 [K][KC][NB][2][64][8] with KC = ceil(Cin/16), NB = ceil(Cout/32),
 * [.][.][.][0] the hi and [1] the lo parts, element [l][j] = W[k][cin = 16 kc +
 * 8 (l >> 5) + j][cout = 32 nb + (l & 31)], zero beyond Cin / Cout.
 *
 * cmt_sparse_to_dense: out [B, C*D, H, W] fp32 (spconv's .dense() [B,C,D,H,W]
 * viewed as the reference does), zero-filled here, out[b][c*D + z][y][x] = X[m][c]. */
typedef struct cmt_sparse_index_args {
    int B, D, H, W;
    int n_cap, reserved;
    const int* coors; const int* count;
    void* index; int64_t index_bytes;
} cmt_sparse_index_args;
typedef struct cmt_sparse_rulebook_args {
    int B, D, H, W;                               /* the input grid */
    int kernel3[3], stride3[3], padding3[3];
    int K;                                        /* kD*kH*kW */
    int n_cap;                                    /* input rows (capacity of coors and of index) */
    int cap;                                      /* down: capacity of the outputs */
    const int* coors; const int* count;
    const void* index; int64_t index_bytes;       /* the input set's index */
    void* out_index; int64_t out_index_bytes;     /* down */
    int* out_coors; int* out_count;               /* down */
    int* nbr;                                     /* subm [n_cap][K]; down [cap][K] */
} cmt_sparse_rulebook_args;
typedef struct cmt_sparse_conv_args {
    int cap, n_in_cap, Cin, Cout, K, relu;
    const float* X; int64_t ldx;
    const int* nbr; const int* count;
    const void* Wp; int64_t wp_bytes;
    const float* scale; const float* shift;       /* [Cout] */
    const float* R; int64_t ldr;                  /* optional residual rows */
    float* Y; int64_t ldy;
} cmt_sparse_conv_args;
typedef struct cmt_sparse_dense_args {
    int B, D, H, W, C, n_cap;
    const float* X; int64_t ldx;
    const int* coors; const int* count;
    float* out;
} cmt_sparse_dense_args;
int64_t cmt_sparse_index_args_size(void);
int64_t cmt_sparse_rulebook_args_size(void);
int64_t cmt_sparse_conv_args_size(void);
int64_t cmt_sparse_dense_args_size(void);
int64_t cmt_sparse_index_bytes(int B, int D, int H, int W, int cap);
int64_t cmt_sparse_pack_bytes(int K, int Cin, int Cout);
int cmt_sparse_index(const cmt_sparse_index_args* args, void* stream);
int cmt_sparse_rulebook_subm(const cmt_sparse_rulebook_args* args, void* stream);
int cmt_sparse_rulebook_down(const cmt_sparse_rulebook_args* args, void* stream);
int cmt_sparse_conv(const cmt_sparse_conv_args* args, void* stream);
int cmt_sparse_to_dense(const cmt_sparse_dense_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Dense BEV backbone and neck (additive to ABI 25): the convolutions of mmdet3d's
 * SECOND (pts_backbone) and SECONDFPN (pts_neck) that cmt_gemm does not cover,
 * inference only, BN folded by the caller (W' = scale * W, shift per channel).
 * Semantics restated from mmdet3d 1.0.0rc6 (models/backbones/second.py,
 * models/necks/second_fpn.py; neither is a dependency):
 *   SECOND    blocks[i] = conv3x3(in_i, out_i, stride s_i, pad 1) BN ReLU, then
 *             layer_nums[i] x [conv3x3(out_i, out_i, pad 1) BN ReLU]
 *   SECONDFPN deblocks[i] = ConvTranspose2d(in_i, out_i, k_i, stride k_i) (or a 1 x 1
 *             Conv2d for k_i = 1) BN ReLU; outputs concatenated along channels
 * The stride-1 convs run on cmt_gemm (CMT_A_CONV3X3_NCHW from the fp32 map,
 * CMT_A_CONV3X3 on pair rows).  Operands here are CMT_F16P rows (leading dimensions
 * in 16-bit words) and split W; arithmetic as the split cmt_gemm: lo*Whi + hi*Wlo +
 * hi*Whi on v_mfma_f32_32x32x16_f16, fp32 accumulation in fixed K order, bitwise
 * repeatable.  range_flag as cmt_gemm_args.range_flag (a pre-activation value that is
 * non-finite or |x| >= 65520 ORs 1 into the word; NULL: off).  No call synchronises
 * with the host.
 *
 * cmt_bev_conv3x3: Y[(b, yo, xo)][n] = act(sum_{ky,kx,c} X[(b, s yo - 1 + ky,
 *   s xo - 1 + kx)][c] * Wt[n][(ky*3 + kx) * Cin + c] + shift[n]), zero outside the
 *   map, Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1 (an odd extent pads both ends of
 *   the strided output, an even one only the low end).  X: NHWC pair rows
 *   [B*H*W][2 Cin]; Wt: pair rows [Cout][2][9 Cin], tap-major K; Y: pair rows
 *   [B*Ho*Wo][2 Cout]; rows beyond B*Ho*Wo are not written.
 *   Requirements: stride 1 or 2, Cin % 32 == 0, Cout % 128 == 0, W <= 180,
 *   ldx, ldw % 8 == 0, X and Wt 16-byte aligned.
 *
 * cmt_bev_deblock: Y[b][c0 + n][k y + dy][k x + dx] = act(sum_c X[(b, y, x)][c] *
 *   Wt[(dy*k + dx) * Cout + n][c] + shift[n]), k in {1, 2, 4} (kernel = stride).
 *   X: pair rows [B*H*W][2 Cin]; Wt: pair rows [k*k*Cout][2][Cin]; Y: fp32 NCHW
 *   [B, Ctot, k H, k W], only channels [c0, c0 + Cout) are written (one writer per
 *   element, stores are runs along x staged through LDS) -- the concatenation of the
 *   neck costs nothing and the result is what CMT_A_CONV3X3_NCHW reads.
 *   Requirements: Cin % 32 == 0, Cout % 128 == 0, c0 + Cout <= Ctot, ldx, ldw % 8 == 0,
 *   X and Wt 16-byte aligned. */
typedef struct cmt_bev_conv_args {
    int B, H, W, Cin, Cout, stride, relu, reserved;
    const void* X; int64_t ldx;
    const void* Wt; int64_t ldw;
    const float* shift;                           /* [Cout] */
    void* Y; int64_t ldy;
    int* range_flag;
} cmt_bev_conv_args;
typedef struct cmt_bev_deblock_args {
    int B, H, W, Cin, Cout, k, c0, Ctot, relu, reserved;
    const void* X; int64_t ldx;
    const void* Wt; int64_t ldw;
    const float* shift;                           /* [Cout] */
    float* Y;
    int* range_flag;
} cmt_bev_deblock_args;
int64_t cmt_bev_conv_args_size(void);
int64_t cmt_bev_deblock_args_size(void);
int cmt_bev_conv3x3(const cmt_bev_conv_args* args, void* stream);
int cmt_bev_deblock(const cmt_bev_deblock_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Camera neck (additive to ABI 25): the two launches of the FPN over the image
 * backbone's maps (img_neck, CPFPN) that cmt_gemm does not cover, inference only, BN
 * folded by the caller.  The 3 x 3 output conv runs on cmt_gemm CMT_A_CONV3X3.
 * Operands and arithmetic as the cmt_bev_* block: CMT_F16P rows (leading dimensions in
 * 16-bit words), split W, lo*Whi + hi*Wlo + hi*Whi on v_mfma_f32_32x32x16_f16 with
 * fp32 accumulation in fixed K order, one writer per element, no atomics on the data
 * path, bitwise repeatable.  No call synchronises with the host.
 *
 * cmt_fpn_lateral: L[(b, y, x)][n] = act(sum_c X[b][c][y][x] * Wt[n][c] + shift[n])
 *   + T[(b, sy(y), sx(x))][n]: a 1 x 1 conv read transposed from the fp32 NCHW map with
 *   the coarser level's nearest-upsampled rows added in the epilogue.
 *   X: fp32 [B][Cin][H*W], channel stride H*W, batch stride x_bstride (floats); every
 *   value is split in registers (hi = f16(x), lo = f16(x - hi)), no pair-row copy of X
 *   is written.  Wt: pair rows [Cout][2][Cin].  T: the coarser level's output of this
 *   same entry, pair rows [B*Htop*Wtop][2 Cout], or NULL for no top-down term; it is
 *   added in fp32 (hi + lo) after the activation and before the output is split.
 *   L: pair rows [B*H*W][2 Cout]; rows beyond B*H*W are not written.
 *   Nearest indices as torch's F.interpolate(size=...): sy(y) = min((int)floorf(y * s),
 *   Htop - 1) with s = (float)Htop / (float)H (one fp32 multiply); sx alike.
 *   range_flag: an input value, a pre-activation value or a pre-split output that is
 *   non-finite or |x| >= 65520 ORs 1 into the word (NULL: off).
 *   Requirements: Cin % 16 == 0, Cout % 128 == 0, x_bstride >= Cin*H*W, with T
 *   1 <= Htop <= H and 1 <= Wtop <= W, ldw >= 2 Cin, ldt, ldl >= 2 Cout, all % 8,
 *   Wt, T and L 16-byte aligned.  H*W is arbitrary.
 *
 * cmt_rows_to_nchw: Y[b][c][p] = (float)hi + (float)lo of pair row b*HW + p, element c:
 *   the inverse of cmt_nchw_to_rows for CMT_F16P rows, through an LDS transpose (loads
 *   along channels, stores along pixels).  X: pair rows [B*HW][2 C] (ldx >= 2 C, % 8,
 *   16-byte aligned); Y: fp32 contiguous [B][C][HW].  C % 8 == 0, HW arbitrary. */
typedef struct cmt_fpn_lateral_args {
    int B, H, W, Cin, Cout, Htop, Wtop, relu;
    const float* X; int64_t x_bstride;
    const void* Wt; int64_t ldw;
    const float* shift;                           /* [Cout] */
    const void* T; int64_t ldt;
    void* L; int64_t ldl;
    int* range_flag;
} cmt_fpn_lateral_args;
typedef struct cmt_rows_to_nchw_args {
    int B, C, HW, reserved;
    const void* X; int64_t ldx;
    float* Y;
} cmt_rows_to_nchw_args;
int64_t cmt_fpn_lateral_args_size(void);
int64_t cmt_rows_to_nchw_args_size(void);
int cmt_fpn_lateral(const cmt_fpn_lateral_args* args, void* stream);
int cmt_rows_to_nchw(const cmt_rows_to_nchw_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Image backbone (additive to ABI 25): the launches of VoVNet-eSE (img_backbone, the
 * non-depthwise specs), inference only, BN folded by the caller.  A map between layers
 * is NHWC CMT_F16P pair rows [B*H*W][2 C] (leading dimensions in 16-bit words);
 * arithmetic of the three GEMM-like kernels as the cmt_bev_* block: lo*Whi + hi*Wlo +
 * hi*Whi on v_mfma_f32_32x32x16_f16, fp32 accumulation in fixed K order, one writer
 * per element, no atomics on the data path, bitwise repeatable.  range_flag: a
 * pre-activation value (stem: also a pixel; apply: the result) that is non-finite or
 * |x| >= 65520 ORs 1 into the word (NULL: off).  No call synchronises with the host.
 * No entry has a width limit; B*H*W < 2^31, byte offsets are 64-bit.
 *
 * cmt_img_stem: Y[(b, yo, xo)][n] = act(sum_{ky,kx,c} X[b][c][2 yo - 1 + ky][2 xo - 1 + kx]
 *   * Wt[n][(ky*3 + kx) * Cin + c] + shift[n]): the 3 x 3 / stride 2 / pad 1 conv straight
 *   from the fp32 NCHW image (channel stride H*W, batch stride x_bstride floats), every
 *   pixel split in registers.  Wt: pair rows [Cout][2][32], K = 9 Cin zero-padded to 32.
 *   Ho = (H - 1) / 2 + 1, Wo alike.  Requirements: 1 <= Cin <= 3, Cout % 32 == 0,
 *   ldy >= 2 Cout, Wt 16-byte aligned.
 *
 * cmt_img_conv3x3: the contract of cmt_bev_conv3x3 (stride 1 or 2, pad 1, pair rows to
 *   pair rows, Wt pair rows [Cout][2][9 Cin] tap-major) without its width limit and with
 *   Cin % 32 == 0, Cout % 32 == 0, Cout <= 256; ldx, ldw % 8 == 0, X and Wt 16-byte
 *   aligned.  A wave owns 32 output rows x 32 nb columns: all Cout (nb = Cout / 32) where the
 *   row tiles alone fill the device, fewer on small maps; nb = 0 lets the entry choose
 *   from the row count and the device's compute units.  The result does not depend on nb.
 *
 * cmt_img_concat1x1: Y[(b, p)][n] = act(sum_s sum_c X_s[(b, p)][c] * Wt[n][off_s + c]
 *   + shift[n]), off_s = C_0 + ... + C_{s-1}: the 1 x 1 conv of a channel concatenation
 *   that is never written.  Up to CMT_IMG_MAX_SRC sources, each pair rows [B*HW][2 C_s]
 *   with its own leading dimension ldx_s >= 2 C_s (a source may be the 2 C_s-word column
 *   slice of a wider row buffer; the words outside it are not read).
 *   Wt: pair rows [Cout][2][K], K = sum C_s.  Tiles of cmt_img_concat_tile_rows() pixels
 *   lie within one image.  part (or NULL): fp32 [B][tiles][Cout], tiles =
 *   ceil(HW / tile rows): the sum over the tile's pixels of the values as stored
 *   ((float)hi + (float)lo after the activation), summed in a fixed order.
 *   Requirements: 1 <= nsrc <= 8, C_s % 32 == 0, Cout % 128 == 0, ldx_s, ldw % 8 == 0,
 *   X_s and Wt 16-byte aligned.
 *
 * cmt_img_ese_gate: gate[b][o] = hsigmoid(sum_c Wfc[o][c] * (sum_t part[b][t][c]) / HW
 *   + bias[o]), hsigmoid(t) = min(max(t + 3, 0), 6) / 6.  fp32 FMA, tiles summed in
 *   ascending order.  Wfc: fp32 [C][C]; gate: fp32 [B][C].  C % 4 == 0, C <= 8192.
 *
 * cmt_img_ese_apply: Y[(b, p)][c] = pair(x * gate[b][c] (+ r)), x and r un-paired as
 *   (float)hi + (float)lo; R NULL: no identity term.  Y may be X.  C % 8 == 0, leading
 *   dimensions % 8, X, R and Y 16-byte aligned.
 *
 * cmt_img_maxpool: 3 x 3 / stride 2 / ceil-mode / no-pad max on pair rows: windows are
 *   clipped at the bottom / right edge, Ho = (H - 2) / 2 + 1, Wo alike.  Values compare
 *   as (float)hi + (float)lo (a NaN wins, as in torch); the winning pair is copied
 *   unchanged, the first of equal maxima in window order.  H, W >= 2, C % 8 == 0. */
#define CMT_IMG_MAX_SRC 8
typedef struct cmt_img_stem_args {
    int B, H, W, Cin, Cout, relu;
    const float* X; int64_t x_bstride;
    const void* Wt;                               /* [Cout][2][32] */
    const float* shift;                           /* [Cout] */
    void* Y; int64_t ldy;
    int* range_flag;
} cmt_img_stem_args;
typedef struct cmt_img_conv_args {
    int B, H, W, Cin, Cout, stride, relu;
    int nb;                                       /* 32-column blocks per workgroup, a divisor of Cout / 32; 0: chosen */
    const void* X; int64_t ldx;
    const void* Wt; int64_t ldw;
    const float* shift;                           /* [Cout] */
    void* Y; int64_t ldy;
    int* range_flag;
} cmt_img_conv_args;
typedef struct cmt_img_concat_args {
    int B, HW, Cout, nsrc, relu, reserved;
    int C[CMT_IMG_MAX_SRC];
    const void* X[CMT_IMG_MAX_SRC];
    int64_t ldx[CMT_IMG_MAX_SRC];
    const void* Wt; int64_t ldw;
    const float* shift;                           /* [Cout] */
    void* Y; int64_t ldy;
    float* part;                                  /* [B][tiles][Cout] or NULL */
    int* range_flag;
} cmt_img_concat_args;
typedef struct cmt_img_gate_args {
    int B, C, tiles, HW;
    const float* part;                            /* [B][tiles][C] */
    const float* Wfc;                             /* [C][C] */
    const float* bias;                            /* [C] */
    float* gate;                                  /* [B][C] */
} cmt_img_gate_args;
typedef struct cmt_img_apply_args {
    int B, HW, C, reserved;
    const void* X; int64_t ldx;
    const float* gate;                            /* [B][C] */
    const void* R; int64_t ldr;
    void* Y; int64_t ldy;
    int* range_flag;
} cmt_img_apply_args;
typedef struct cmt_img_pool_args {
    int B, H, W, C;
    const void* X; int64_t ldx;
    void* Y; int64_t ldy;
} cmt_img_pool_args;
int64_t cmt_img_stem_args_size(void);
int64_t cmt_img_conv_args_size(void);
int64_t cmt_img_concat_args_size(void);
int64_t cmt_img_gate_args_size(void);
int64_t cmt_img_apply_args_size(void);
int64_t cmt_img_pool_args_size(void);
int cmt_img_concat_tile_rows(void);
int cmt_img_stem(const cmt_img_stem_args* args, void* stream);
int cmt_img_conv3x3(const cmt_img_conv_args* args, void* stream);
int cmt_img_concat1x1(const cmt_img_concat_args* args, void* stream);
int cmt_img_ese_gate(const cmt_img_gate_args* args, void* stream);
int cmt_img_ese_apply(const cmt_img_apply_args* args, void* stream);
int cmt_img_maxpool(const cmt_img_pool_args* args, void* stream);

/* ------------------------------------------------------------------------
 * Image backbone, the one-pass fp16 policy (additive to ABI 25): the launches above on
 * plain fp16 rows.  A map between layers is NHWC [B*H*W][C] of IEEE fp16 (leading
 * dimensions in 16-bit words, half of the pair rows'); weights are BN-folded and rounded
 * once to fp16 by the caller, the shift stays fp32.  Every 16-k step is one
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation in fixed K order (the K order of the
 * entries above); the epilogue adds the shift, applies the activation and rounds once to
 * fp16 (RNE; |x| >= 65520 stores an infinity and raises range_flag).  fp16 subnormal
 * operands are kept by the MFMA, not flushed.  One writer per element, no atomics on
 * the data path, bitwise repeatable, no scratch, no call synchronises with the host.
 * The argument structs are those above with the leading dimensions halved; range_flag as
 * above.  cmt_img_ese_gate is shared: it reads fp32 partial sums either way.
 *
 * cmt_img_stem_f16: cmt_img_stem with every pixel rounded to fp16 on load and
 *   Wt: fp16 [Cout][32], K = 9 Cin zero-padded to 32.  Requirements: 1 <= Cin <= 3,
 *   Cout % 32 == 0, ldy >= Cout and % 8, Wt 16-byte aligned.
 *
 * cmt_img_conv3x3_f16: cmt_img_conv3x3 on fp16 rows; Wt: fp16 [Cout][9 Cin] tap-major
 *   (k = (ky*3 + kx) * Cin + c).  Cin % 32 == 0, Cout % 32 == 0, Cout <= 256, stride 1 or
 *   2, pad 1; ldx >= Cin, ldw >= 9 Cin, ldy >= Cout, all % 8; X and Wt 16-byte aligned.
 *   W is staged 64 k per chunk; Cin % 64 == 32 ends every tap in a half chunk.  nb as in
 *   cmt_img_conv3x3: 0 lets the entry choose, the result does not depend on it.
 *
 * cmt_img_concat1x1_f16: cmt_img_concat1x1 on up to CMT_IMG_MAX_SRC fp16 sources
 *   [B*HW][C_s] with ldx_s >= C_s (a source may be a C_s-word column slice of a wider
 *   row buffer); Wt: fp16 [Cout][K], K = sum C_s.  part (or NULL): fp32 [B][tiles][Cout],
 *   the fp32 sums over the tile's pixels of the fp16 values as stored, in the fixed
 *   order of cmt_img_concat1x1.  Requirements: 1 <= nsrc <= 8, C_s % 32 == 0,
 *   Cout % 128 == 0, ldx_s >= C_s, ldw >= K, ldy >= Cout, all % 8; X_s and Wt 16-byte
 *   aligned.
 *
 * cmt_img_ese_apply_f16: Y[(b, p)][c] = f16(x * gate[b][c] (+ r)), computed in fp32 and
 *   rounded once; R NULL: no identity term.  Y may be X.  C % 8 == 0, ldx, ldr, ldy >= C
 *   and % 8, X, R, Y and gate 16-byte aligned.
 *
 * cmt_img_maxpool_f16: cmt_img_maxpool's windows on fp16 values: the winning element is
 *   copied unchanged, the first of equal maxima in window order, a NaN wins.  H, W >= 2,
 *   C % 8 == 0, ldx, ldy >= C and % 8, X and Y 16-byte aligned.
 *
 * cmt_rows_to_nchw_f16 (fpn.hip): Y[b][c][p] = (float)X[b*HW + p][c], fp16 rows to
 *   contiguous fp32 [B][C][HW] through the LDS transpose of cmt_rows_to_nchw.
 *   C % 8 == 0, ldx >= C and % 8, X 16-byte aligned, HW arbitrary. */
int cmt_img_stem_f16(const cmt_img_stem_args* args, void* stream);
int cmt_img_conv3x3_f16(const cmt_img_conv_args* args, void* stream);
int cmt_img_concat1x1_f16(const cmt_img_concat_args* args, void* stream);
int cmt_img_ese_apply_f16(const cmt_img_apply_args* args, void* stream);
int cmt_img_maxpool_f16(const cmt_img_pool_args* args, void* stream);
int cmt_rows_to_nchw_f16(const cmt_rows_to_nchw_args* args, void* stream);

/* ---- camera frames -> the image backbone's input (imgprep.hip; additive to ABI 25) ----------------
 * cmt_img_prepare: the test-time image pipeline of the reference (integer crop of
 * ResizeCropFlipImage at resize 1, NormalizeMultiviewImage, PadMultiViewImage) in one pass.
 *   src: uint8 [N][Hs][Ws][3], contiguous and interleaved (any byte alignment).
 *   dst: fp32 [N][3][Hp][Wp], contiguous, 4-byte aligned (16-byte stores when Wp % 4 == 0 and
 *   dst is 16-byte aligned, scalar stores otherwise); every element is written.
 *   For y < h and x < w, with b the byte of source pixel (y0 + y, x0 + x), channel
 *   (to_rgb ? 2 - c : c), or 0 where that pixel lies outside the source:
 *     dst[n][c][y][x] = fl32(fl32((float)b - mean[c]) * inv_std[c]);
 *   dst[n][c][y][x] = 0 for y >= h or x >= w.  inv_std is the caller's float32 reciprocal of std.
 *   Requirements: N, Hs, Ws, w, h > 0, Hp >= h, Wp >= w, |x0|, |y0|, Hp, Wp < 2^30,
 *   N * Hp * ceil(Wp / 4) < 2^31 (element offsets are 64-bit); CMT_EINVAL otherwise. */
typedef struct cmt_img_prepare_args {
    int N, Hs, Ws, to_rgb;
    int x0, y0, w, h;                             /* crop window in source pixels */
    int Hp, Wp;
    float mean[3], inv_std[3];                    /* by destination channel */
    const void* src;
    void* dst;
} cmt_img_prepare_args;
int64_t cmt_img_prepare_args_size(void);
int cmt_img_prepare(const cmt_img_prepare_args* args, void* stream);

/* cmt_img_resize_prepare (additive to ABI 25): cmt_img_prepare with "source" replaced by "the source
 * resized to Hr x Wr", i.e. ResizeCropFlipImage(training=False) at any resize_dims, then normalise
 * and pad, in one launch.  Layouts, alignment rules, to_rgb, the pad and the limits are
 * cmt_img_prepare's; additionally Hr, Wr > 0 and < 2^30.  The window (x0, y0, w, h) is in pixels of
 * the resized image.  For y < h and x < w, with b the byte of RESIZED pixel (y0 + y, x0 + x),
 * channel (to_rgb ? 2 - c : c), or 0 where that pixel lies outside [0, Hr) x [0, Wr):
 *     dst[n][c][y][x] = fl32(fl32((float)b - mean[c]) * inv_std[c]);   0 for y >= h or x >= w.
 * The resized byte is the 8-bit fixed-point bilinear sample written down here (a restatement from
 * memory of OpenCV's plain C++ INTER_LINEAR path; THIS TEXT is the contract, agreement with a real
 * cv2.resize has not been verified).  Per axis, source size S, resized size R, resized index d:
 *     scale = (double)S / R;
 *     f = (float)((d + 0.5) * scale - 0.5)   float64 multiply, then float64 subtract (no FMA), one
 *                                            rounding to float32;
 *     s = floor(f), t = f - s                float32;
 *     horizontal axis only: s < 0 -> s = 0, t = 0;  s >= S - 1 -> s = S - 1, t = 0;
 *     c1 = rint(t * 2048), c0 = rint((1.f - t) * 2048)    float32, round-half-even;
 *     taps at clamp(s, 0, S - 1) and clamp(s + 1, 0, S - 1)   (the vertical axis only clamps).
 * With (a0, a1) / (b0, b1) the horizontal / vertical coefficients, taps s, s' and rows r0, r1, per
 * channel k in int32:
 *     Hrow_r = src[r][s][k] * a0 + src[r][s'][k] * a1
 *     byte   = (((b0 * (Hrow_r0 >> 4)) >> 16) + ((b1 * (Hrow_r1 >> 4)) >> 16) + 2) >> 2
 * c0 + c1 == 2048 always, so constants are preserved, R == S reproduces the source and an exact
 * 2 x downscale is the rounded mean of 4 pixels.  The call never synchronises and allocates nothing. */
typedef struct cmt_img_resize_args {
    int N, Hs, Ws, to_rgb;
    int Hr, Wr;                                   /* the size the frame is resized to */
    int x0, y0, w, h;                             /* crop window in pixels of the resized image */
    int Hp, Wp;
    float mean[3], inv_std[3];                    /* by destination channel */
    const void* src;
    void* dst;
} cmt_img_resize_args;
int64_t cmt_img_resize_args_size(void);
int cmt_img_resize_prepare(const cmt_img_resize_args* args, void* stream);

/* ---- the training-side image pipeline (imgaug.hip; additive to ABI 25) ----------------------------
 * THIS TEXT is the contract of the three entry points below: a restatement of the reference's host
 * pipeline in which every rounding is fixed.  The parts that restate OpenCV (cv2.warpAffine,
 * cv2.getRotationMatrix2D, cv2.resize) and PIL (Image.rotate by 0 degrees, taken as the identity) are
 * written from memory; agreement with a real OpenCV or PIL has NOT been verified.  Every CMT_EINVAL
 * condition is checked before any device work; no call synchronises with the host or allocates.
 *
 * cmt_img_augment: ResizeCropFlipImage[Coop](training=True) fused with NormalizeMultiviewImage and
 * PadMultiViewImage, optionally with GridMask and the image branch of ModalMask3D, in one launch.
 *   src: uint8 [N][Hs][Ws][3], contiguous (any byte alignment).  dst: fp32 [N][3][Hp][Wp], contiguous,
 *   4-byte aligned (16-byte stores when Wp % 4 == 0 and dst is 16-byte aligned, scalar stores
 *   otherwise); every element is written.  The crop size (w, h) is shared (final_dim); image n carries
 *   img[n] = (Hr, Wr, x0, y0, flip, zero, iM[6]): the size it is resized to, the origin of its crop
 *   window in resized pixels, the horizontal flip, ModalMask3D's "0. * img", and the inverse affine
 *   map of the rotation (destination pixel -> pixel of the flipped crop), row-major 2 x 3.
 *   For y < h and x < w the value before normalisation is
 *     AX = rint(iM[0] * x * 1024)            AY = rint(iM[3] * x * 1024)
 *     BX = rint((iM[1] * y + iM[2]) * 1024) + 16
 *     BY = rint((iM[4] * y + iM[5]) * 1024) + 16
 *          float64 products and sums, each rounded on its own (no FMA), rint = round-half-even
 *     X = (BX + AX) >> 5,  Y = (BY + AY) >> 5     arithmetic shifts
 *     ix = X >> 5, fx = X & 31, iy = Y >> 5, fy = Y & 31
 *     val = ((32-fx)(32-fy) T(iy,ix) + fx(32-fy) T(iy,ix+1) + (32-fx)fy T(iy+1,ix) + fx fy T(iy+1,ix+1)) / 1024
 *   (cv2.warpAffine(crop, M, (w, h)), INTER_LINEAR, constant border 0, on the float64 crop the reference
 *   builds: positions quantised to 1/32 pixel, exact weights).  The integers are evaluated in 64 bits:
 *   with |iM[k]| < 2^20 and w, h < 2^30 none exceeds 2^61, so nothing wraps.  val is a multiple of
 *   1/1024 below 256 and its float32 form is exact.  The identity iM = {1,0,0, 0,1,0} gives fx = fy = 0,
 *   ix = x, iy = y: an exact pass-through.
 *   The caller's iM for a rotation by a degrees about (cx, cy) = (w / 2, h / 2) (native_imgaug.warp_inverse;
 *   cv2.getRotationMatrix2D((cx, cy), a, 1), then cv2.warpAffine's own inversion), all in float64, in this
 *   order of operations:
 *     r = a * (pi / 180);  al = cos(r);  be = sin(r)
 *     M = { al, be, (1 - al) * cx - be * cy,   -be, al, be * cx + (1 - al) * cy }
 *     D = M[0] * M[4] - M[1] * M[3];  D = (D != 0) ? 1 / D : 0
 *     A11 = M[4] * D;  A22 = M[0] * D;  M[0] = A11;  M[1] *= -D;  M[3] *= -D;  M[4] = A22
 *     b1 = -M[0] * M[2] - M[1] * M[5];  b2 = -M[3] * M[2] - M[4] * M[5];  M[2] = b1;  M[5] = b2;  iM = M
 *   (b1 and b2 use the updated M[0], M[1], M[3], M[4]).  a == 0 passes the identity itself, not this sequence.
 *   Tap T(ty, tx): 0 outside [0, h) x [0, w).  Otherwise, with tx' = flip ? w - 1 - tx : tx, the resized
 *   pixel (y0 + ty, x0 + tx'): 0 outside [0, Hr) x [0, Wr), else the byte of cmt_img_resize_prepare's
 *   8-bit bilinear (source Hs x Ws resized to Hr x Wr) at that pixel, channel (to_rgb ? 2 - c : c).
 *   With zero set every tap is 0.
 *     dst[n][c][y][x] = fl32(fl32(val - mean[c]) * inv_std[c]);   0 for y >= h or x >= w.
 *   GridMask: with grid.d > 0 every element of dst, the pad included, is then multiplied by
 *   m(y, x) in {0.f, 1.f} and the float32 product is stored (a masked negative value stores -0.f):
 *     hh = (int)(1.5 * Hp), ww = (int)(1.5 * Wp)    float64 product, truncated
 *     Y = y + (hh - Hp) / 2, X = x + (ww - Wp) / 2  integer division
 *     rowband = Y >= st_h && (Y - st_h) / d < hh / d && (Y - st_h) % d < l
 *     colband = X >= st_w && (X - st_w) / d < ww / d && (X - st_w) % d < l
 *     base = !((use_h && rowband) || (use_w && colband));   m = (mode == 1) ? !base : base
 *   the reference's GridMask.forward for rotate == 1 (its only value in the configs: r = 0) and
 *   offset == False; the mask is shared by the N images.  grid.d == 0: no mask.
 *   CMT_EINVAL: a null struct, src or dst; N outside 1..CMT_IMG_AUG_MAX; Hs, Ws, w, h <= 0; Hp < h;
 *   Wp < w; Hs, Ws, w, h, Hp, Wp >= 2^30; Hp * ceil(Wp / 4) >= 2^31; dst not 4-byte aligned; a NaN
 *   mean or inv_std; per image Hr, Wr <= 0 or >= 2^30, |x0| or |y0| >= 2^30, a non-finite iM[k] or
 *   |iM[k]| >= 2^20; grid.d < 0, or with grid.d > 0: d < 2, d >= 2^30, l < 1, l >= d, st_h or st_w
 *   outside [0, d).
 *
 * cmt_grid_mask: the same predicate (Hp = h, Wp = w) applied in place to fp32 [planes][h][w]
 *   (planes = n * c of a prepared batch): x[p][y][x] = fl32(x[p][y][x] * m(y, x)).  16-byte accesses
 *   when w % 4 == 0 and x is 16-byte aligned, scalar ones otherwise.
 *   CMT_EINVAL: a null struct or x; x not 4-byte aligned; planes, h or w <= 0; h, w >= 2^30;
 *   planes * h * ceil(w / 4) >= 2^31; the grid conditions above with d > 0 required.
 *
 * cmt_img_paste: the pixel part of unified_sample (sample_2d=True) in place on uint8 frames
 *   [N][Hs][Ws][3], before cmt_img_augment.  Camera n has an ordered list of count[n] rectangles
 *   (x0, y0, x1, y1, crop), half-open as the reference's slices are, 0 <= x0 <= x1 <= Ws and
 *   0 <= y0 <= y1 <= Hs; crop = -1 marks a box of the frame's own ground truth, crop >= 0 indexes the
 *   patch table (offset, hc, wc): patch bytes [hc][wc][3] at patch_bytes + offset.  The tables are given
 *   twice: rects / patches in HOST memory (rects is [N][CMT_PASTE_MAX_RECTS], only the first count[n]
 *   of a row are read), which the entry validates and from which it takes each camera's bounding
 *   rectangle, and rects_dev / patches_dev, the caller's device copies of the same bytes, which the
 *   kernel reads.  The kernel writes only inside the bounding rectangle taken from the host table and
 *   skips a device entry that fails the host-side conditions, so a stale device copy cannot make it
 *   touch memory outside the frames and the patch buffer.
 *   For every pixel, with v its 3 bytes, walk the camera's list in order over the rectangles that
 *   contain it; m = mixup, om = 1 - m in float64, computed once on the host:
 *     raw box (crop == -1):  m < 0: v unchanged;  m >= 0: v = trunc(fl64(v * om) + fl64(v * m)).
 *       (The reference's saved crops are numpy VIEWS of the frame, not copies, so its "restitching"
 *       reads the current pixel, whatever was pasted over it before; this is what the line above says.)
 *     sampled box, patch not empty (hc > 0 and wc > 0): c = the patch resized to (x1 - x0) x (y1 - y0)
 *       by the 8-bit bilinear of cmt_img_resize_prepare (S = wc / hc, R = x1 - x0 / y1 - y0), sampled
 *       at (x - x0, y - y0);  m < 0: v = c;  m >= 0: v = trunc(fl64(v * om) + fl64(c * m)).
 *     sampled box with an empty patch: skipped.
 *   Products and the sum are separate float64 roundings (no FMA), per channel; trunc is the conversion
 *   to uint8 of a value in [0, 255].  Pixels outside every rectangle are not written.  Each pixel is
 *   read and written by one thread only, so the update in place is safe.
 *   CMT_EINVAL: a null struct or frames; N outside 1..CMT_IMG_AUG_MAX; Hs, Ws <= 0 or >= 2^30; a
 *   count[n] outside [0, CMT_PASTE_MAX_RECTS]; with any rectangle: null rects, rects_dev; a rectangle
 *   outside the frame or with x1 < x0 or y1 < y0; crop < -1 or >= n_patches; n_patches < 0; with
 *   n_patches > 0: null patches, patches_dev or patch_bytes; a patch with hc < 0, wc < 0, hc or wc
 *   >= 2^15, offset < 0 or offset + 3 * hc * wc > patch_bytes_size; mixup NaN or > 1 (mixup < 0: plain
 *   paste); a camera's bounding rectangle of 2^31 or more 64 x 4 pixel tiles. */
#define CMT_IMG_AUG_MAX 16
#define CMT_PASTE_MAX_RECTS 256
typedef struct cmt_grid_params {
    int d, l, st_h, st_w;                         /* d == 0: no mask (cmt_img_augment only) */
    int use_h, use_w, mode, reserved;
} cmt_grid_params;
typedef struct cmt_img_aug_image {
    int Hr, Wr;                                   /* the size this frame is resized to */
    int x0, y0;                                   /* crop origin in pixels of the resized frame */
    int flip, zero;
    double iM[6];                                 /* inverse affine map of the rotation, row-major 2 x 3 */
} cmt_img_aug_image;
typedef struct cmt_img_augment_args {
    int N, Hs, Ws, to_rgb;
    int w, h, Hp, Wp;                             /* shared crop size and padded size */
    float mean[3], inv_std[3];                    /* by destination channel */
    cmt_grid_params grid;
    cmt_img_aug_image img[CMT_IMG_AUG_MAX];
    const void* src;
    void* dst;
} cmt_img_augment_args;
typedef struct cmt_grid_mask_args {
    int64_t planes;
    int h, w;
    cmt_grid_params grid;
    void* x;
} cmt_grid_mask_args;
typedef struct cmt_paste_rect { int x0, y0, x1, y1, crop; } cmt_paste_rect;
typedef struct cmt_paste_patch { int64_t offset; int hc, wc; } cmt_paste_patch;
typedef struct cmt_img_paste_args {
    int N, Hs, Ws, n_patches;
    int count[CMT_IMG_AUG_MAX];                   /* rectangles per camera */
    double mixup;                                 /* < 0: plain paste */
    const cmt_paste_rect* rects;                  /* host [N][CMT_PASTE_MAX_RECTS] */
    const cmt_paste_patch* patches;               /* host [n_patches] */
    const void* rects_dev;                        /* device copy of rects */
    const void* patches_dev;                      /* device copy of patches */
    const void* patch_bytes;                      /* device, packed uint8 patches */
    int64_t patch_bytes_size;
    void* frames;                                 /* device uint8 [N][Hs][Ws][3], updated in place */
} cmt_img_paste_args;
int64_t cmt_img_augment_args_size(void);
int64_t cmt_grid_mask_args_size(void);
int64_t cmt_img_paste_args_size(void);
int cmt_img_augment(const cmt_img_augment_args* args, void* stream);
int cmt_grid_mask(const cmt_grid_mask_args* args, void* stream);
int cmt_img_paste(const cmt_img_paste_args* args, void* stream);

/* ---- raw LiDAR sweeps -> the detector's points (ptsprep.hip; additive to ABI 25) -------------------
 * cmt_pts_prepare: the point side of the reference's test pipeline for ONE cloud (one agent's key frame
 * plus its sweeps): LoadPointsFromMultiSweeps[Coop] (remove_close, sweep -> key-frame transform, time
 * column, concatenation, use_dim), VehiclePointsToInfraCoords and PointsRangeFilter[Coop], as an
 * order-preserving stream compaction.  THIS TEXT is the contract: a restatement of the reference in which
 * every rounding is fixed.
 *   src: fp32 [n_total][load_dim], contiguous, 4-byte aligned (rows are read dword by dword), load_dim 3..8.
 *   S segments, 1 <= S <= CMT_PTS_MAX_SEG: segment s holds rows [seg_start[s], seg_start[s + 1]), with
 *   seg_start[0] == 0, seg_start non-decreasing and seg_start[S] == n_total.  Empty segments and
 *   n_total == 0 are legal; n_total < 2^31 (element offsets are 64-bit).
 *   dst: fp32 [n_total][F_out], contiguous, 4-byte aligned, F_out 3..8; count: one device int32.
 * Per row of segment s, in this order (x, y, z = columns 0, 1, 2 of the raw row; fl32 = one rounding to
 * float32, round-to-nearest-even; no operation below is fused with another):
 *   1. remove_close, on the raw row: with r = close_radius > 0 the row is dropped iff |x| < r && |y| < r
 *      in float32.  A NaN compares false, so such a row is kept (as numpy does).  r == 0: off.
 *   2. sweep transform (has_sweep_xform), numpy's float64 matrix on a float32 array, for k = 0, 1, 2:
 *        q_k = fl32(((double)x * rot[3k] + (double)y * rot[3k + 1]) + (double)z * rot[3k + 2])
 *      float64 products and float64 sums, left to right, no FMA; then
 *        p_k = fl32((double)q_k + trans[k]).
 *      rot is sensor2lidar_rotation row-major (the reference's pts[:, :3] @ rot.T), trans its translation.
 *   3. time column: time_col >= 0 sets column time_col of the row to time_val (the host's
 *      fl32(ts - sweep_ts) for a sweep, 0 for the key frame); time_col == -1 leaves the row as it is.
 *   4. column selection: out[j] = row[use_dim[j]], j < F_out.  use_dim[0..2] must be 0, 1, 2.
 *   5. agent transform (has_agent_xform), mmdet3d's BasePoints.rotate(R.T) then translate(t) in float32
 *      on out[0..2], with rot32 = R row-major (the vehicle2infrastructure rotation) and trans32 = t:
 *        p'_k = fl32(fl32(fl32(fl32(x * rot32[3k]) + fl32(y * rot32[3k + 1])) + fl32(z * rot32[3k + 2])) + trans32[k])
 *      The reference's float32 matmul leaves the order of its sums to the BLAS; this text fixes one.
 *   6. range filter (has_range), in_range_3d: the row is kept iff out[k] > range[k] && out[k] < range[3 + k]
 *      for k = 0, 1, 2, strict, in float32; a NaN or +-inf coordinate drops the row.  Without the filter
 *      such rows are kept.
 * Kept rows go to dst[0 .. count) in input order (segment order, then row order: the reference's cat);
 * rows [count, n_total) are filled with the quiet NaN 0x7FC00000 in every column, so every element of dst
 * is written and a voxelizer that drops non-finite points sees the trimmed cloud.  count is written once.
 * Two launches (per-tile kept counts of cmt_pts_prepare_tile_rows() rows into the workspace; then prefix,
 * scatter and fill), no workgroup waits for another, no host synchronisation, no allocation:
 * graph-capturable.  The workspace (cmt_pts_prepare_workspace_bytes(n_total) bytes, 4-byte aligned) is
 * rewritten by every call before it is read: it needs no initialisation and no cleaning, and serves one
 * stream at a time.  Each workgroup of the second launch reads every tile count, so the call is meant for
 * clouds of up to a few million rows.
 * CMT_EINVAL, before any device work: S, load_dim, F_out or use_dim out of range; seg_start[0] != 0,
 * decreasing, or seg_start[S] != n_total; n_total < 0 or >= 2^31; time_col < -1 or >= load_dim;
 * close_radius negative or non-finite; a non-finite transform that is switched on; range non-finite or
 * min >= max; src, dst or workspace null or misaligned with n_total > 0; count null; workspace_bytes
 * below cmt_pts_prepare_workspace_bytes(n_total). */
#define CMT_PTS_MAX_SEG 16
typedef struct cmt_pts_segment {
    double rot[9], trans[3];                      /* sweep -> key frame, float64 as the info files hold them */
    int has_sweep_xform;
    float close_radius;                           /* 0: off */
    int time_col;                                 /* -1: leave the column */
    float time_val;
} cmt_pts_segment;
typedef struct cmt_pts_prepare_args {
    int64_t n_total;
    int S, load_dim, F_out;
    int has_agent_xform, has_range, reserved;
    int64_t seg_start[CMT_PTS_MAX_SEG + 1];
    int use_dim[8];
    float rot32[9], trans32[3];                   /* agent transform */
    float range[6];                               /* x, y, z min, then x, y, z max */
    cmt_pts_segment seg[CMT_PTS_MAX_SEG];
    const void* src;
    void* dst;
    int* count;
    void* workspace;
    int64_t workspace_bytes;
} cmt_pts_prepare_args;
int64_t cmt_pts_prepare_args_size(void);
int64_t cmt_pts_prepare_workspace_bytes(int64_t n_total);   /* 0 for n_total <= 0 */
int cmt_pts_prepare_tile_rows(void);
int cmt_pts_prepare(const cmt_pts_prepare_args* args, void* stream);

/* ---- detection evaluation: nuScenes-style AP / TP errors on the device (deteval.hip; additive to ABI 25) ----
 * The reference's in-tree evaluator (a9coop_dataset.py accumulate / cummean / calc_ap / calc_tp /
 * filter_eval_boxes) for boxes that already live on the device.  THIS TEXT is the contract.  All arithmetic
 * is float64 on the float32 inputs, every product, sum, quotient and square root is rounded on its own
 * (no FMA), sums run left to right as written.
 *
 * Inputs.  Predictions: N rows of box[9] fp32 (x, y, z, w, l, h, yaw, vx, vy), score fp32, label int32,
 * sample int32, in arrival order (the reference's list index).  Ground truth: G rows of box[9] fp32, label,
 * sample, num_pts int32 (-1: unknown), the rows of one sample in annotation order (rows of different samples
 * may interleave).  N and G are capacities: with n_pred / n_gt non-null only rows below that device word
 * (clamped to [0, capacity]) exist.  A row whose label is outside [0, C) or whose sample is outside [0, S)
 * does not exist either.  Scores must not be NaN (a NaN score is ordered by its bit pattern).
 * Config: C <= 32 classes with range[c] and yaw_period[c], T <= 8 thresholds dist_th[t], tp_index (the
 * position of dist_th_tp), first_ind = round(100 * min_recall) + 1 in [1, 100], min_precision in [0, 1).
 *
 * Filters.  A row is kept iff sqrt(x * x + y * y) < range[label] (strict; NaN drops it); a ground-truth row
 * additionally only if num_pts != 0.
 * Order.  Within a class predictions are visited by descending score, equal scores (-0 equals +0) by
 * descending row index.
 * Match, per (class c, threshold t): the visited prediction takes, among the not yet taken kept ground truth
 * of its sample and class, the one with the smallest d = sqrt(dx * dx + dy * dy) (dx, dy: centre
 * differences); equal d: the lowest annotation index.  tp = 1 iff d < dist_th[t] (strict), and only then is
 * that ground truth taken (for this t alone) and match_gt = its row; else tp = 0, match_gt = -1.
 * Errors of a match (prediction p, ground truth g), NaN for a row without one:
 *   err[0] trans = d;   err[1] vel = sqrt(dvx * dvx + dvy * dvy);
 *   err[2] scale = 1 - i / ((vg + vp) - i), v = (w * l) * h, i = (min(wg, wp) * min(lg, lp)) * min(hg, hp),
 *          min as numpy.minimum (a NaN operand gives NaN);
 *   err[3] orient = |diff|, diff = pymod((yaw_g - yaw_p) + P / 2, P) - P / 2, then diff -= 2 pi if diff > pi;
 *          pymod(a, P) = fmod(a, P), plus P when that is negative (Python's %), P = yaw_period[c] > 0.
 * Curves, per (c, t).  npos[c] = kept ground truth of the class; the class's kept predictions in visiting
 * order are j = 0 .. n - 1, ctp[j] the inclusive running count of tp, M = ctp[n - 1].  npos == 0 or M == 0
 * (n == 0 included) gives the "no predictions" block: recall r, precision = confidence = 0, the four errors 1.
 * Otherwise, with r_k = k * 0.01 (r_100 = 1), rec[j] = ctp[j] / npos, prec[j] = ctp[j] / (j + 1):
 *   precision = interp(r, rec, prec, right = 0), confidence = interp(r, rec, score, right = 0);
 *   each error curve e: value_k = interp(confidence_k, mc reversed, cm_e reversed), where mc[m] is the score
 *   of the m-th match in visiting order and cm_e the NaN-aware cumulative mean of err[e] over the matches:
 *   (sum of the non-NaN values up to m) / (their count), 0 while the count is 0, and 1 everywhere when all
 *   are NaN.  The cumulative sums use a fixed tree (8 consecutive terms per thread, a wave scan, the waves,
 *   the 2048-term chunks in order); two runs are bit-equal.
 *   interp(x, xp, fp) is numpy.interp: j = the largest index with xp[j] <= x; x > xp[last]: right (default
 *   fp[last]); x < xp[0]: fp[0]; j == last or xp[j] == x: fp[j]; else
 *   ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])) * (x - xp[j]) + fp[j].
 * Scalars.  ap[c][t] = mean over k >= first_ind of max(precision_k - min_precision, 0), divided by
 * (1 - min_precision).  tp_err[c][e], from the t = tp_index curves: with last_ind the last k of non-zero
 * confidence (0 if none), 1 when last_ind < first_ind, else the mean of the error curve over
 * [first_ind, last_ind].  Means are serial sums in index order divided by the count.
 *
 * Three stream-ordered calls on one args struct, with two sorts by the caller between the first two:
 *   cmt_det_eval_keys   writes the int64 sort keys key_class[N], key_sample[N] (both for row N - 1 - j at
 *                       position j, so that a STABLE ascending sort visits equal scores by descending row) and
 *                       key_gt[G] (row j at position j).  Rows that do not exist or are filtered get INT64_MAX.
 *                       key_class = class << 32 | ~ord(score), key_sample = (sample << 6 | class) << 32 |
 *                       ~ord(score), key_gt = sample << 6 | class; ord() is the order-preserving uint32 of a float.
 *   the caller sorts each key array ascending and stable and passes the sorted keys and the int64 indices
 *   (sk_class / si_class, sk_sample / si_sample, sk_gt / si_gt).
 *   cmt_det_eval_match  one wave per (sample, class): tp[T][N] uint8, match_gt[T][N] int32, err[T][4][N]
 *                       float64 and npos[C]; every element is written by exactly one lane, no atomics.
 *   cmt_det_eval_curves one workgroup per (class, threshold): md[C][T][7][101] float64 (recall, precision,
 *                       confidence, trans, vel, scale, orient), ap[C][T], tp_err[C][4].
 * No host synchronisation and no allocation inside.  The workspace (cmt_det_eval_workspace_bytes, 8-byte
 * aligned) needs no initialisation.  CMT_EINVAL before any device work: N or G outside [0, 2^31), S outside
 * [1, 2^24], C outside [1, 32], T outside [1, 8], tp_index outside [0, T), first_ind outside [1, 100],
 * min_precision outside [0, 1), a non-finite or non-positive range, yaw_period or dist_th, a null or
 * misaligned pointer that the call uses, a short workspace. */
#define CMT_DET_MAX_CLASSES 32
#define CMT_DET_MAX_THRESHOLDS 8
#define CMT_DET_NELEM 101
typedef struct cmt_det_eval_args {
    int64_t N, G;                                  /* capacities (rows) */
    int S, C, T, tp_index, first_ind, reserved;
    double range[CMT_DET_MAX_CLASSES], yaw_period[CMT_DET_MAX_CLASSES], dist_th[CMT_DET_MAX_THRESHOLDS];
    double min_precision;
    const void *pred_box, *pred_score, *pred_label, *pred_sample;
    const void *gt_box, *gt_label, *gt_sample, *gt_num_pts;
    const int *n_pred, *n_gt;                      /* device words, or null: all rows */
    void *key_class, *key_sample, *key_gt;         /* int64 [N], [N], [G]: written by cmt_det_eval_keys */
    const void *sk_class, *si_class, *sk_sample, *si_sample, *sk_gt, *si_gt;   /* int64, sorted keys and indices */
    void *tp, *match_gt, *err, *npos;              /* written by cmt_det_eval_match */
    void *md, *ap, *tp_err;                        /* written by cmt_det_eval_curves */
    void* workspace;
    int64_t workspace_bytes;
} cmt_det_eval_args;
int64_t cmt_det_eval_args_size(void);
int64_t cmt_det_eval_workspace_bytes(int64_t N, int64_t G, int S, int C, int T);   /* -1 for arguments out of range */
int cmt_det_eval_keys(const cmt_det_eval_args* args, void* stream);
int cmt_det_eval_match(const cmt_det_eval_args* args, void* stream);
int cmt_det_eval_curves(const cmt_det_eval_args* args, void* stream);

/* ---- IoU-matched detection AP (deteval.hip, box_overlap.h; additive to ABI 25) ------------------------
 * The same evaluation with overlap in place of the centre distance (KITTI / VOC style).  Filters, order,
 * keys, sorts, output layouts, errors and curves are those above; cmt_det_eval_match_iou stands where
 * cmt_det_eval_match stands, and cmt_det_eval_ap_interp adds the interpolated APs after (or without)
 * cmt_det_eval_curves:  keys -> the three sorts -> match_iou -> curves -> ap_interp.
 * Overlap.  For a visited prediction p and a kept ground truth g of its sample and class, iou(p, g) is
 * cmt_box_iou's float32 value with THE GROUND TRUTH AS THE FIRST BOX (the pair is clipped in g's frame, so
 * the value of a ground truth does not depend on which prediction asks): mode 0 its bev, mode 1 its iou3d,
 * both with z_origin.  A box that is invalid there (a non-finite field among the first seven, or a
 * non-positive extent) gives 0 on either side; a NaN quotient (0 / 0 of underflowed extents) counts as 0.
 * Match, per (class c, threshold t): the visited prediction takes, among the not yet taken kept ground truth
 * of its sample and class, the one with the LARGEST iou; equal iou: the lowest annotation index.  tp = 1 iff
 * iou > iou_th[t] (strict, in float32: an iou of 0 never matches), and only then is that ground truth taken
 * (for this t alone) and match_gt = its row; else tp = 0, match_gt = -1.  The four errors of a match are the
 * ones above, err[0] still the centre distance in float64.  match_iou[T][N] (optional) is the iou of the
 * match, NaN without one.  dist_th of the base struct is validated but not read.
 * Every output element has exactly one writer, no atomics, no memset: two runs are bit-equal.
 * Interpolated APs, per (c, t), with ctp, prec, n, M, npos as above: env[j] = max over k >= j of prec[k],
 * pos(m) the position of the m-th match (m = 1 .. M):
 *   ap_interp[c][t][0]  all-point AP = (sum over m of env[pos(m)], a serial sum in m order) / npos;
 *   ap_interp[c][t][1]  R40 = (sum over k = 1 .. 40, in k order, of env[pos(m_k)]) / 40, m_k the smallest m
 *                       with m * 40 >= k * npos (integers), the term 0 when m_k > M;
 *   both 0 when npos == 0 or M == 0.  Float64; a maximum does not round, the sums are serial: bit-equal.
 * cmt_det_eval_ap_interp reads tp, npos and the sorted class keys and uses the workspace of the base struct.
 * CMT_EINVAL before any device work: whatever cmt_det_eval_match refuses in the base struct, a mode other
 * than 0 / 1, a z_origin other than 0 / 0.5, an iou_th outside [0, 1) or non-finite, a misaligned match_iou,
 * a null or misaligned ap_interp (cmt_det_eval_ap_interp only). */
typedef struct cmt_det_iou_args {
    int mode, reserved;                       /* 0 BEV, 1 3D */
    float z_origin;                           /* 0 or 0.5, as cmt_box_iou */
    float iou_th[CMT_DET_MAX_THRESHOLDS];     /* T of them, each in [0, 1) */
    void* match_iou;                          /* fp32 [T][N], or null */
    void* ap_interp;                          /* float64 [C][T][2], for cmt_det_eval_ap_interp */
} cmt_det_iou_args;
int64_t cmt_det_iou_args_size(void);
int cmt_det_eval_match_iou(const cmt_det_eval_args* args, const cmt_det_iou_args* iou, void* stream);
int cmt_det_eval_ap_interp(const cmt_det_eval_args* args, const cmt_det_iou_args* iou, void* stream);

/* ---- training-side point and box pipeline (ptsaug.hip; additive to ABI 25) ---------------------------
 * The chain every reference config that trains on points runs between loading and the voxelizer:
 * [Unified]ObjectSample[Coop] (the part after the database sampler has chosen its objects),
 * GlobalRotScaleTransAll[Coop], CustomRandomFlip3D, PointsRangeFilter[Coop], ObjectRangeFilter,
 * ObjectNameFilter and PointShuffle[Coop].  THIS TEXT is the contract: a restatement in which every rounding
 * is fixed.  The conventions are mmdet3d v1.0.0rc6's as the reference calls them (BasePoints.rotate / scale /
 * translate / flip, LiDARInstance3DBoxes.rotate / scale / translate / flip / in_range_bev / limit_yaw,
 * box_np_ops.points_in_rbbox); they have not been compared with an installed mmdet3d.
 * fl32 = one rounding to float32, round-to-nearest-even; no operation below is fused with another.
 * All three calls: caller-owned buffers, stream-ordered, no host synchronisation, no allocation, no
 * workgroup waits for another: graph-capturable.  Every output element has exactly one writer, the counts
 * of cmt_points_in_boxes excepted (integer atomics).  Inputs and outputs must not overlap.
 *
 * A LiDAR box is a row of D fp32, D 7 or 9: x, y, z_bottom, dx, dy, dz, yaw [, vx, vy].
 * The inside test of a point p and a box, in real arithmetic:
 *   d = p - (x, y, z_bottom),  lx = d.x * cos(yaw) + d.y * sin(yaw),  ly = -d.x * sin(yaw) + d.y * cos(yaw),
 *   inside iff |lx| < dx / 2 && |ly| < dy / 2 && 0 < d.z && d.z < dz, all strict
 * (points_in_rbbox with the bottom-centre origin (0.5, 0.5, 0): the open interior).  A NaN anywhere in the
 * point or the box gives "outside"; so does dx, dy or dz <= 0.  The kernels evaluate it in float32 with
 * the device's sinf / cosf, one pair per box: the contract binds only points farther than
 * 1e-4 * (1 + max |coordinate|) metres from every face plane of every box (max over the point and the
 * box centre); nearer ones may fall on either side, the same side in both launches of cmt_pts_augment.
 *
 * The transform parameters (cmt_aug_xform), applied where a step below names them:
 *   rotation (has_rot): rot32 = R row-major, R = [[c, -s, 0], [s, c, 0], [0, 0, 1]] for the angle a
 *     (counter-clockwise, p' = R p: BasePoints.rotate(a)), built by the caller in float64 and rounded once;
 *     angle32 = fl32(a).  For k = 0, 1, 2, the arithmetic of cmt_pts_prepare step 5 without the translation:
 *       p'_k = fl32(fl32(fl32(x * rot32[3k]) + fl32(y * rot32[3k + 1])) + fl32(z * rot32[3k + 2]))
 *   scale (has_scale): p_k = fl32(p_k * scale).   translation (has_trans): p_k = fl32(p_k + trans32[k]).
 *   flip_h ('horizontal'): y = -y.   flip_v ('vertical'): x = -x.   (sign changes, exact)
 *   range (has_range): x, y, z min, then x, y, z max.
 *
 * cmt_points_in_boxes: N points fp32 [N][F], F 3..8 (columns 0..2 are read), M boxes fp32 [M][D].
 *   count_in: null, or a device int32 clamped to [0, N]: rows at or beyond it belong to no box.
 *   box_of_point int32 [N] (null: skipped): the lowest index of a box that contains the point, -1 for none.
 *   count_per_box int32 [M] (null: skipped): zeroed by the call, then every containing box is incremented
 *   (points_in_rbbox(...).sum(0)) with integer atomics, at most one per wave and box.
 *   Boxes are staged per workgroup cmt_points_in_boxes_chunk() at a time; a workgroup owns
 *   cmt_pts_augment_tile_rows() consecutive points.  N == 0 and M == 0 are legal; N < 2^31, M < 2^24.
 *   CMT_EINVAL before any device work: N, M, F or D out of range; points null or misaligned with N > 0;
 *   boxes null or misaligned with M > 0; a misaligned count_in, box_of_point or count_per_box.
 *
 * cmt_pts_augment: one cloud.  src fp32 [n_src][F] with the optional device count_in (clamped to
 *   [0, n_src]; the padded pair of cmt_pts_prepare), paste fp32 [n_paste][F] (the sampled objects' points),
 *   paste_boxes fp32 [K][7], K <= CMT_AUG_MAX_BOXES, order int32 [n_in] or null, n_in = n_src + n_paste < 2^31.
 *   The concatenated index space is the paste rows then the src rows (paste_first != 0: ObjectSampleCoop)
 *   or the src rows then the paste rows (UnifiedObjectSample[Coop], points.cat([points, sampled])).
 *   Slot j = 0 .. n_in - 1 visits row i = order ? order[j] : j; an i outside [0, n_in) drops the slot.
 *   Per visited row, in this order:
 *     1. a src row at or beyond *count_in is dropped;
 *     2. remove_points_in_boxes: a src row inside any paste box (the inside test above) is dropped; paste
 *        rows are never tested;
 *     3. rotation, 4. scale, 5. translation, 6. flips, on columns 0..2 as written above;
 *     7. in_range_3d (has_range): kept iff p_k > range[k] && p_k < range[3 + k], k = 0, 1, 2, strict, float32;
 *        a NaN or +-inf coordinate drops the row.  Without the filter such rows are kept.
 *   Columns 3 and beyond are copied bit for bit.  Kept rows go to dst[0 .. count) in slot order; rows
 *   [count, n_in) of dst fp32 [n_in][F] are the quiet NaN 0x7FC00000 in every column; count is written once.
 *   PointShuffle needs no sort: a uniform permutation of all rows restricted to the kept rows is a uniform
 *   shuffle of the kept rows, so the caller passes a random permutation as order.
 *   Two launches, as cmt_pts_prepare (per-tile kept counts of cmt_pts_augment_tile_rows() slots; then prefix,
 *   scatter and fill); the workspace (cmt_pts_augment_workspace_bytes(n_in) bytes, 4-byte aligned) is
 *   rewritten by every call before it is read.  shift_height is not built.
 *   CMT_EINVAL before any device work: F outside 3..8; K outside [0, CMT_AUG_MAX_BOXES]; n_src, n_paste
 *   negative or n_in >= 2^31; shift_height != 0; a non-finite rotation, angle, scale, translation or range
 *   that is switched on; range min >= max; count null or misaligned; with rows present a null or misaligned
 *   src (n_src > 0), paste (n_paste > 0), paste_boxes (K > 0), dst or workspace (n_in > 0); a misaligned
 *   count_in or order; workspace_bytes below cmt_pts_augment_workspace_bytes(n_in).
 *
 * cmt_boxes_augment: the same parameters on the annotations (the ground truth followed by the pasted boxes,
 *   concatenated by the caller): boxes fp32 [n][D], labels int64 [n] -> out_boxes fp32 [n][D], out_labels
 *   int64 [n], count (device int32).  One workgroup; n <= CMT_AUG_MAX_ANN.  Per box, in this order:
 *     rotation (has_rot): the centre (columns 0..2) like a point; yaw = fl32(yaw + angle32); D == 9:
 *       vx' = fl32(fl32(vx * rot32[0]) + fl32(vy * rot32[1])), vy' = fl32(fl32(vx * rot32[3]) + fl32(vy * rot32[4]));
 *     scale: columns 0..5 and 7..8;   translation: columns 0..2;
 *     flip_h: columns 1 and 8 negated, yaw = -yaw;
 *     flip_v: columns 0 and 7 negated, yaw = fl32(fl32(-yaw) + fl32(pi));
 *     ObjectRangeFilter (has_range), in_range_bev: kept iff x > range[0] && y > range[1] && x < range[3] &&
 *       y < range[4], strict, float32 (a NaN drops the box);
 *     ObjectNameFilter: a label < 0 or >= num_classes drops the box;
 *     limit_yaw(0.5, 2 pi): yaw = fl32(yaw - fl32(floorf(fl32(fl32(yaw / P) + 0.5f)) * P)), P = fl32(2 pi),
 *       the division correctly rounded;
 *     gravity != 0: column 2 = fl32(z + fl32(dz * 0.5f)) (the head's gravity-centre layout).
 *   Kept boxes and their labels go to rows [0, count) in input order; rows [count, n) are quiet NaN / -1.
 *   CMT_EINVAL before any device work: n outside [0, CMT_AUG_MAX_ANN]; D not 7 or 9; num_classes < 0; the
 *   transform conditions of cmt_pts_augment; count null or misaligned; with n > 0 a null or misaligned (boxes
 *   and out_boxes 4 bytes, labels 8 bytes) buffer. */
#define CMT_AUG_MAX_BOXES 128
#define CMT_AUG_MAX_ANN 65536
typedef struct cmt_aug_xform {
    int has_rot, has_scale, has_trans, flip_h, flip_v, has_range;
    float rot32[9], angle32, scale;
    float trans32[3], range[6];
} cmt_aug_xform;
typedef struct cmt_points_in_boxes_args {
    int64_t N;
    int M, F, D, reserved;
    const void* points;
    const int* count_in;
    const void* boxes;
    int* box_of_point;
    int* count_per_box;
} cmt_points_in_boxes_args;
typedef struct cmt_pts_augment_args {
    int64_t n_src, n_paste;
    int F, K, paste_first, shift_height;
    cmt_aug_xform xf;
    const void* src;
    const int* count_in;
    const void* paste;
    const void* paste_boxes;
    const int* order;
    void* dst;
    int* count;
    void* workspace;
    int64_t workspace_bytes;
} cmt_pts_augment_args;
typedef struct cmt_boxes_augment_args {
    int n, D, num_classes, gravity;
    cmt_aug_xform xf;
    const void* boxes;
    const void* labels;
    void* out_boxes;
    void* out_labels;
    int* count;
} cmt_boxes_augment_args;
int64_t cmt_points_in_boxes_args_size(void);
int64_t cmt_pts_augment_args_size(void);
int64_t cmt_boxes_augment_args_size(void);
int cmt_points_in_boxes_chunk(void);
int cmt_pts_augment_tile_rows(void);
int64_t cmt_pts_augment_workspace_bytes(int64_t n_in);   /* 0 for n_in <= 0 */
int cmt_points_in_boxes(const cmt_points_in_boxes_args* args, void* stream);
int cmt_pts_augment(const cmt_pts_augment_args* args, void* stream);
int cmt_boxes_augment(const cmt_boxes_augment_args* args, void* stream);

/* ---- ground-truth database (gtdb.hip; additive to ABI 25) ---------------------------------------------
 * What create_groundtruth_database builds and UnifiedDataBaseSampler / sample_class_v2 do with it, without
 * the files: the points of every annotated box as a segment of one device buffer, the BEV collision test
 * with its greedy loop, and the gather of the chosen segments into the paste rows of cmt_pts_augment.
 * THIS TEXT is the contract.  The conventions are mmdet3d v1.0.0rc6's as the reference calls them
 * (box_np_ops.points_in_rbbox, box_np_ops.center_to_corner_box2d, data_augment_utils.box_collision_test,
 * dbsampler.BatchSampler); they are not compared with an installed mmdet3d.
 * fl32 = one rounding to float32; no operation below is fused with another.
 * All three calls: caller-owned buffers, stream-ordered, no allocation, no host synchronisation, no
 * workgroup waits for another: graph-capturable.  Every output element has exactly one writer and there are
 * no atomics: results are bitwise repeatable.  Inputs and outputs must not overlap.
 *
 * cmt_gtdb_extract: one frame.  points fp32 [N][F], F 3..8; count_in null or a device int32 clamped to
 *   [0, N] (rows at or beyond it belong to no box); boxes fp32 [M][D], D 7 or 9, M <= CMT_GTDB_MAX_BOXES,
 *   N < 2^31 and N * M < 2^31.  rows fp32 [cap][F], offsets int32 [M + 1].
 *   Row i of the cloud belongs to segment b iff the inside test of the section above holds for point i and
 *   box b, evaluated with the instructions of cmt_points_in_boxes: it binds only points farther than
 *   1e-4 * (1 + max |coordinate|) metres from every face plane of every box (max over the point and the box
 *   centre); nearer ones may fall on either side, the same side as in cmt_points_in_boxes and in every launch
 *   of this call.  A NaN in the point or the box, or dx, dy or dz <= 0, gives "outside".  A point inside
 *   several boxes appears in each of them (points[point_indices[:, b]]).
 *   offsets[b] = the number of (point, box) hits of the boxes < b; offsets[M] = the total, never capped.
 *   Segment b is rows [offsets[b], offsets[b + 1]) in cloud order.  Columns 0..2 of a row are
 *   fl32(p_k - box_k), k = 0, 1, 2, with box_2 = z_bottom (gt_points[:, :3] -= gt_boxes_3d[b, :3]); columns 3
 *   and beyond are copied bit for bit.  A destination row at or beyond cap is not written; nothing outside
 *   rows [0, min(total, cap)) is touched, and cap == 0 (rows may be null) gives the offsets alone.
 *   Three launches: the hits of every (tile, box) pair over tiles of cmt_pts_augment_tile_rows() points,
 *   boxes staged cmt_points_in_boxes_chunk() at a time; one workgroup that scans them; a scatter that
 *   evaluates the same function again and skips every (tile, box chunk) pair without a hit.  The workspace
 *   (cmt_gtdb_extract_workspace_bytes(N, M) bytes, 4-byte aligned) is rewritten by every call before it is read.
 *   CMT_EINVAL before any device work: N, N * M, M, F, D or cap (outside [0, 2^31)) out of range; points
 *   null or misaligned with N > 0; boxes null or misaligned with M > 0; offsets null or misaligned; a
 *   misaligned count_in or rows; rows null with cap > 0; with N, M > 0 a null or misaligned workspace or
 *   workspace_bytes below cmt_gtdb_extract_workspace_bytes(N, M).
 *
 * cmt_gtdb_gather: K <= CMT_AUG_MAX_BOXES segments in one launch.  rows fp32 [n_rows][F] (segments as
 *   cmt_gtdb_extract writes them), device int32 tables seg_offset, seg_len, dst_offset [K], centre fp32 [K][3],
 *   dst fp32 [n_dst][F].  For k < K and i < seg_len[k]: dst[dst_offset[k] + i] = rows[seg_offset[k] + i] with
 *   columns 0..2 fl32(v + centre[k][c]) (s_points.translate(info['box3d_lidar'][:3])) and the rest copied bit
 *   for bit.  The segments must not overlap in dst (one writer per row).  A source row outside [0, n_rows)
 *   or a destination row outside [0, n_dst) moves nothing.
 *   CMT_EINVAL before any device work: K, F, n_rows or n_dst out of range; a misaligned buffer; with K > 0
 *   a null table or centre; with K, n_rows, n_dst > 0 a null rows or dst.
 *
 * cmt_gtdb_collide: boxes fp32 [n][D], n = n_gt + n_s <= CMT_GTDB_MAX_COLLIDE: n_gt boxes to avoid, then n_s
 *   candidates.  group: a HOST int32 [n_s], non-decreasing, read before the call returns: the sample_class_v2
 *   call (the class) each candidate belongs to.  keep int32 [n_s] (0 / 1) and count (device int32) are written.
 *   Corners (center_to_corner_box2d, origin 0.5), float32, one sinf / cosf pair (s, c) per box, for k = 0..3
 *   with (sx, sy) = (-,-), (-,+), (+,+), (+,-):  lx = sx * fl32(dx * 0.5f),  ly = sy * fl32(dy * 0.5f),
 *     X_k = fl32(fl32(fl32(lx * c) - fl32(ly * s)) + x),   Y_k = fl32(fl32(fl32(lx * s) + fl32(ly * c)) + y)
 *   (counter-clockwise by yaw, the rotation sense of the inside test).  The stand-up rectangle of a box is
 *   the min and max of its X_k and of its Y_k.
 *   collide(P, Q) is box_collision_test(..., clockwise=True) for the pair, every difference, product and
 *   comparison in float32:
 *     iw = fl32(min(P.xmax, Q.xmax) - max(P.xmin, Q.xmin)); not iw > 0: no.  ih likewise in y; not ih > 0: no.
 *     For the edges (A, B) = (P_k, P_k+1) and (C, D) = (Q_l, Q_l+1), k and l 0..3 (indices mod 4), k outer:
 *       acd = (D.y - A.y) * (C.x - A.x) > (C.y - A.y) * (D.x - A.x)
 *       bcd = (D.y - B.y) * (C.x - B.x) > (C.y - B.y) * (D.x - B.x)
 *       abc = (C.y - A.y) * (B.x - A.x) > (B.y - A.y) * (C.x - A.x)
 *       abd = (D.y - A.y) * (B.x - A.x) > (B.y - A.y) * (D.x - A.x)
 *       acd != bcd && abc != abd: yes (the edges cross).
 *     Otherwise yes iff P contains Q or, failing that, Q contains P.  "P contains Q": for every corner Q_l and
 *     every edge k of P, with v = P_k+1 - P_k:
 *       cross = fl32(fl32(v.y * (P_k.x - Q_l.x)) - fl32(v.x * (P_k.y - Q_l.y))) < 0   (cross >= 0 ends it)
 *   The greedy loop takes the candidates in order.  Candidate i is rejected iff collide(i, j) for a live box
 *   j != i, and then leaves the live set at once (the reference clears its row and column); otherwise it is
 *   kept.  Live are: every box to avoid; a kept candidate of an earlier group; a candidate of i's own group
 *   that has not been rejected yet, later ones included.  count = the number kept.
 *   The contract binds only scenes in which every comparison the sequential evaluation above makes (with its
 *   early exits) has |lhs - rhs| > tol = 2^-16 * (1 + Cmax) * (1 + Emax), Cmax the largest |corner
 *   coordinate| and Emax the largest box diagonal of the scene; boxes must be finite.  One workgroup; the
 *   matrix collide(candidate, any box) is kept as bits in LDS (32 KB at n = 512) and one wave runs the loop.
 *   CMT_EINVAL before any device work: n_gt or n_s negative or n_gt + n_s > CMT_GTDB_MAX_COLLIDE; D not 7 or
 *   9; with n_s > 0 a null group or one that decreases; count null or misaligned; boxes null or misaligned
 *   with n > 0; keep null or misaligned with n_s > 0. */
#define CMT_GTDB_MAX_BOXES 1024
#define CMT_GTDB_MAX_COLLIDE 512
typedef struct cmt_gtdb_extract_args {
    int64_t N, cap;
    int M, F, D, reserved;
    const void* points;
    const int* count_in;
    const void* boxes;
    void* rows;
    int* offsets;
    void* workspace;
    int64_t workspace_bytes;
} cmt_gtdb_extract_args;
typedef struct cmt_gtdb_gather_args {
    int64_t n_rows, n_dst;
    int K, F;
    const void* rows;
    const int* seg_offset;
    const int* seg_len;
    const int* dst_offset;
    const void* centre;
    void* dst;
} cmt_gtdb_gather_args;
typedef struct cmt_gtdb_collide_args {
    int n_gt, n_s, D, reserved;
    const void* boxes;
    const int* group;   /* host */
    int* keep;
    int* count;
} cmt_gtdb_collide_args;
int64_t cmt_gtdb_extract_args_size(void);
int64_t cmt_gtdb_gather_args_size(void);
int64_t cmt_gtdb_collide_args_size(void);
int64_t cmt_gtdb_extract_workspace_bytes(int64_t N, int M);   /* 0 for N <= 0 or M <= 0 */
int cmt_gtdb_extract(const cmt_gtdb_extract_args* args, void* stream);
int cmt_gtdb_gather(const cmt_gtdb_gather_args* args, void* stream);
int cmt_gtdb_collide(const cmt_gtdb_collide_args* args, void* stream);

/* ---- multi-object tracker (track.hip; additive to ABI 25) ----------------------------------------------
 * Links the boxes of one frame (cmt_box_decode's rows) to tracks with stable ids: a constant-velocity
 * Kalman filter per axis in the ground plane, a gated squared-distance cost matrix, cmt_lsap between the two
 * calls below, and the tracks' life cycle.  A frame is cmt_track_predict -> cmt_lsap (P = 1, max_nq = T,
 * max_ngt = D, cost_elems = T * D, both match_q [D] and match_g [T]) -> cmt_track_update: five small launches and
 * cmt_lsap's memset of its status word, no host read, no synchronisation; the host knows only T and D, the live and detection counts travel in
 * lsap_desc in device memory.  THIS TEXT is the contract.  fl32 = one rounding to float32; every sum,
 * difference, product and quotient below is an IEEE single operation rounded on its own (none is fused), in
 * the order the parentheses give, a + b + c meaning (a + b) + c; "a += b" is a = fl32(a + b).
 * The assignment minimises the SUM OF SQUARED ground-plane distances over the gated pairs, not the sum of
 * distances: a stated choice that keeps the contract free of a square root.
 * Caller-owned buffers, stream-ordered, no allocation, no workgroup waits for another: graph-capturable.
 * Every output element has one writer and there are no atomics: results are bitwise repeatable.  Buffers must
 * not overlap.  Limits (CMT_ENOTSUP beyond): T <= CMT_TRACK_MAX_TRACKS, D <= CMT_TRACK_MAX_DETS, H <=
 * CMT_TRACK_MAX_HISTORY, ncls <= CMT_TRACK_MAX_CLASSES.
 *
 * State, on the device, a slot is stable for the life of a track:
 *   trk_f fp32 [T][16]: x y z dx dy dz yaw vx vy score Px_pp Px_pv Px_vv Py_pp Py_pv Py_vv
 *   trk_i int32 [T][8]: id (-1: a free slot), label, hits, misses, age, det (the row matched or born from
 *                        in the last update, else -1), hist_n (positions appended since birth), reserved 0
 *   hist  fp32 [T][H][3]: a ring, a position goes to hist[s][hist_n % H]
 *   counters int32 [4]:  n_alive, next_id, births dropped for lack of a slot (cumulative), frames
 *   A fresh state has every id -1 and everything else zero.
 *
 * cmt_track_predict.  det fp32 [D][ld], ld >= 9, columns x y z dx dy dz yaw vx vy; scores fp32 [D]; labels
 *   int32 [D]; count null (n_det = D) or a device int32 clamped to [0, D]; gate2 fp32 [ncls] on the device,
 *   the squared gate per class (the caller keeps every entry below 1e5: the C side cannot read it); pose: with
 *   has_pose != 0 twelve floats, row-major [R|t] (Rab = pose[4a + b], ta = pose[4a + 3]), and pose_yaw.  The
 *   kernels call no trigonometric function.  In order:
 *   1. n_det from count.
 *   2. det_w fp32 [D][9], all D rows: the nine columns copied bit for bit without a pose; with one
 *        x' = ((R00 * x + R01 * y) + R02 * z) + t0, y' and z' likewise with rows 1 and 2,
 *        vx' = R00 * vx + R01 * vy,  vy' = R10 * vx + R11 * vy,  sizes unchanged,
 *        yaw' = yaw + pose_yaw, then yaw' -= 6.2831855f if yaw' >= 3.1415927f, else yaw' += 6.2831855f if
 *        yaw' < -3.1415927f (one conditional step).
 *   3. det_ok int32 [D]: 1 iff j < n_det, the nine values of det_w[j] are finite, 0 <= labels[j] < ncls and
 *      scores[j] >= score_thr (a NaN score gives 0); else 0.
 *   4. every slot with id >= 0, per axis a in {x, y} with (p, v, Ppp, Ppv, Pvv) the axis' five values:
 *        p += dt * v;  t1 = Ppv + dt * Pvv;  Ppp = (Ppp + dt * (Ppv + t1)) + q_pos * dt;  Ppv = t1;
 *        Pvv = Pvv + q_vel * dt;  and age += 1.  Nothing else of the state is written.
 *   5. live int32 [T]: live[r] = the r-th slot with id >= 0 in ascending slot order, r < n_live.
 *   6. cost fp32, row stride D, for r < n_live and j < n_det only, s = live[r]:
 *        d2 = (x_s - x_j) * (x_s - x_j) + (y_s - y_j) * (y_s - y_j)   (predicted state, det_w)
 *        cost = d2 iff det_ok[j], labels[j] == label_s and d2 < gate2[labels[j]]; else CMT_TRACK_BIG.
 *      A non-finite d2 fails the comparison: every cost is finite and cmt_lsap's status is 0.
 *   7. lsap_desc int64 [4] = (0, n_live, n_det, D).
 *   Two launches: one workgroup for 1..5 and 7 (the live list is a ballot / mbcnt scan per 64 slots and an LDS
 *   table over them), then the cost matrix over tiles of 16 rows x 256 columns.
 *   CMT_EINVAL before any device work: a null struct; T, D or ncls < 1; ld < 9; dt, q_pos or q_vel negative or
 *   not finite; score_thr NaN; has_pose with a non-finite pose or pose_yaw; a null or misaligned (4 bytes,
 *   lsap_desc 8) trk_f, trk_i, det, scores, labels, gate2, det_w, det_ok, live, cost or lsap_desc; a
 *   misaligned count.
 *
 * cmt_track_update.  live, lsap_desc, cost, det_w, det_ok as cmt_track_predict wrote them, match_g int32 [T]
 *   and match_q int32 [D] as cmt_lsap wrote them, the scores and labels of cmt_track_predict.  n_live and
 *   n_det are read from lsap_desc and clamped to [0, T] and [0, D].  In order:
 *   1. Row r < n_live with s = live[r] is matched to j iff s is the r-th slot with id >= 0 (the kernel scans
 *      the ids again), j = match_g[r] is in [0, n_det), match_q[j] == r, det_ok[j] and cost[r][j] < CMT_TRACK_BIG.
 *      Entries outside their ranges match nothing and move nothing: a corrupt table cannot write out of bounds,
 *      two rows cannot claim one detection nor one slot.
 *   2. A matched slot, per axis, measurement zp = det_w[j] x / y and zv = det_w[j] vx / vy, every right-hand
 *      side reading the predicted values:
 *      use_velocity != 0:
 *        Spp = Ppp + r_pos, Spv = Ppv, Svv = Pvv + r_vel, det = Spp * Svv - Spv * Spv,
 *        K00 = (Ppp * Svv - Ppv * Spv) / det,  K01 = (Ppv * Spp - Ppp * Spv) / det,
 *        K10 = (Ppv * Svv - Pvv * Spv) / det,  K11 = (Pvv * Spp - Ppv * Spv) / det,
 *        yp = zp - p, yv = zv - v,  p += K00 * yp + K01 * yv,  v += K10 * yp + K11 * yv,
 *        Ppp' = Ppp - (K00 * Ppp + K01 * Ppv), Ppv' = Ppv - (K00 * Ppv + K01 * Pvv),
 *        Pvv' = Pvv - (K10 * Ppv + K11 * Pvv)
 *      use_velocity == 0 (position only):
 *        S = Ppp + r_pos, K0 = Ppp / S, K1 = Ppv / S, y = zp - p,  p += K0 * y,  v += K1 * y,
 *        Ppp' = Ppp - K0 * Ppp, Ppv' = Ppv - K0 * Ppv, Pvv' = Pvv - K1 * Ppv
 *      then z, dx, dy, dz, yaw from det_w[j] and score from scores[j] bit for bit, hits += 1, misses = 0,
 *      det = j, hist[s][hist_n % H] = the updated (x, y, z), hist_n += 1.
 *   3. Every other slot with id >= 0: misses += 1, det = -1; with misses > max_age the slot is freed (id = -1,
 *      nothing else of it changes).
 *   4. Births: the k-th j in ascending order with j < n_det, det_ok[j], not matched and scores[j] >= birth_thr
 *      takes the k-th free slot in ascending slot order, slots freed in step 3 included: id = next_id + k,
 *      label = labels[j]; x y z dx dy dz yaw from det_w[j], (vx, vy) from det_w[j] with use_velocity, else 0;
 *      score; P = (p0_pos, 0, p0_vel) per axis; hits 1, misses 0, age 0, det j, hist[s][0] = (x, y, z),
 *      hist_n 1, reserved 0.  Births beyond the free slots are dropped, counted, and use no id.
 *   5. counters: n_alive = the slots with id >= 0 now, next_id += the births placed, counters[2] += the
 *      births dropped, frames += 1.
 *   6. det_track int32 [D] and det_slot int32 [D], all D entries: the id and slot matched or born for j, else -1.
 *   One launch, one workgroup: the free-slot list and the birth ranks are ballot / mbcnt scans per 64 entries
 *   with an LDS table over them.
 *   CMT_EINVAL before any device work: a null struct; T, D or H < 1; max_age < 0; r_pos or r_vel not finite or
 *   <= 0; p0_pos or p0_vel not finite or negative; birth_thr NaN; a null or misaligned (4 bytes, lsap_desc 8)
 *   pointer. */
#define CMT_TRACK_MAX_TRACKS 512
#define CMT_TRACK_MAX_DETS 1024
#define CMT_TRACK_MAX_HISTORY 32
#define CMT_TRACK_MAX_CLASSES 32
#define CMT_TRACK_BIG 1.0e6f
typedef struct cmt_track_predict_args {
    int T, D, ld, ncls;
    int has_pose, reserved;
    float dt, q_pos, q_vel, score_thr;
    float pose[12];
    float pose_yaw, reserved_f;
    void* trk_f;
    int* trk_i;
    const void* det;
    const void* scores;
    const int* labels;
    const int* count;
    const void* gate2;
    void* det_w;
    int* det_ok;
    int* live;
    void* cost;
    int64_t* lsap_desc;
} cmt_track_predict_args;
typedef struct cmt_track_update_args {
    int T, D, H, use_velocity;
    int max_age, reserved;
    float r_pos, r_vel, p0_pos, p0_vel, birth_thr, reserved_f;
    void* trk_f;
    int* trk_i;
    void* hist;
    int* counters;
    const int* live;
    const int64_t* lsap_desc;
    const void* cost;
    const int* match_g;
    const int* match_q;
    const void* det_w;
    const void* scores;
    const int* labels;
    const int* det_ok;
    int* det_track;
    int* det_slot;
} cmt_track_update_args;
int64_t cmt_track_predict_args_size(void);
int64_t cmt_track_update_args_size(void);
int cmt_track_predict(const cmt_track_predict_args* args, void* stream);
int cmt_track_update(const cmt_track_update_args* args, void* stream);

/* ---- rotated-box IoU, NMS and the candidate set of late fusion (boxiou.hip; additive to ABI 25) ----------
 * How much two boxes overlap, greedy rotated NMS of one box set, and the concatenation of several agents' boxes
 * in one frame.  THIS TEXT is the contract.  fl32 = one rounding to float32; every sum, difference, product and
 * quotient below is an IEEE single operation rounded on its own (none is fused), in the order the parentheses
 * give.  Caller-owned buffers and workspaces, stream-ordered, no allocation, no host read: graph-capturable.  No
 * workgroup waits for another and there are no atomics: results are bitwise repeatable.  Buffers must not
 * overlap.  Every CMT_EINVAL below is returned before any device work.
 *
 * Box rows: fp32 [n][ld], ld >= 7, columns x y z dx dy dz yaw, later columns ignored.  z_origin in {0, 0.5} says
 * what z is: 0.5 the gravity centre (cmt_box_decode's rows, the evaluator's, the tracker's), 0 the bottom
 * (LiDARInstance3DBoxes.tensor).  A row is INVALID if one of its seven values is not finite or dx, dy or dz <= 0:
 * it overlaps nothing, its IoU with every row is exactly 0.  Derived values of a valid row, one sinf / cosf pair
 * per box:
 *   hx = dx * 0.5f, hy = dy * 0.5f, s = sinf(yaw), c = cosf(yaw), bot = z - z_origin * dz, top = bot + dz,
 *   area = dx * dy, vol = area * dz.
 *
 * The overlap of a pair (A, B) is computed IN A'S OWN FRAME: the result does not depend on where in the scene
 * the pair sits, and A's edges are axis-parallel, so identical boxes have no near-parallel edge intersections.
 *   t = (xB - xA, yB - yA);   o = (t.x * cA + t.y * sA,  t.y * cA - t.x * sA)        (B's centre in A's frame)
 *   c = cB * cA + sB * sA;    s = sB * cA - cB * sA                                  (the relative rotation)
 *   corners k = 0..3 with (sx, sy) = (-,-), (-,+), (+,+), (+,-), the order of cmt_gtdb_collide:
 *     lx = sx * hxB, ly = sy * hyB,  X_k = (lx * c - ly * s) + o.x,  Y_k = (lx * s + ly * c) + o.y
 *   The quadrilateral is clipped (Sutherland-Hodgman) against x <= hxA, x >= -hxA, y <= hyA, y >= -hyA, in that
 *   order.  One half-plane with bound b on coordinate u (v the other coordinate), input vertices V_0..V_n-1:
 *   for i = 0..n-1 with p = V_i, q = V_(i+1) mod n: emit p if p is inside; then, if exactly one of p and q is
 *   inside, emit the crossing (u, v) = (b, p.v + ((b - p.u) / (q.u - p.u)) * (q.v - p.v)).  Inside is u <= b
 *   (u >= b for the lower bounds).  The divisor is never 0 and the clipped coordinate is the bound itself.  A
 *   list holds at most 8 vertices; an emission beyond the eighth is dropped (it cannot occur for a convex input).
 *   area = |sum over i = 1..n-2 of ((V_i - V_0) x (V_i+1 - V_0))| * 0.5f, the terms added in ascending i, each
 *     cross product (a.x * b.y) - (a.y * b.x); 0 with fewer than 3 vertices.
 *   bev   = area / ((areaA + areaB) - area)
 *   h     = max(0, min(topA, topB) - max(botA, botB))
 *   iou3d = (area * h) / ((volA + volB) - area * h)
 *
 * cmt_box_iou.  a [N][lda], b [M][ldb]; n_a, n_b: null (N, M) or device int32 words clamped to [0, N] and
 *   [0, M].  bev and / or iou3d fp32 [N][ldo], ldo >= M; either may be null, not both.  Element (i, j) for
 *   i < n_a, j < n_b is written exactly once; nothing else is written.  aligned != 0: M == N, the outputs are
 *   [N], element i is row i of a against row i of b, for i < min(n_a, n_b); ldo is ignored.
 *   One lane per pair over tiles of 64 x 64: 256 threads, a lane owns a column and walks 16 rows; the derived
 *   values of the tile's boxes are computed once per workgroup and staged in LDS; a lane's polygon lives in an
 *   LDS slot of its own (32 KB a workgroup), not in scratch.
 *   CMT_EINVAL: a null struct; N or M < 0; lda or ldb < 7; z_origin not 0 or 0.5; bev and iou3d both null;
 *   aligned with N != M; ldo < M (not aligned); more than 2^31 tiles; a misaligned (4 bytes) pointer; a or b null
 *   with N, M > 0.  N == 0 or M == 0 is a valid call that launches nothing.
 *
 * cmt_box_nms.  Greedy rotated NMS of boxes [N][ld], scores fp32 [N], labels int32 [N] or null, N <=
 *   CMT_NMS_MAX; count null (N) or a device int32 clamped to [0, N].  A row EXISTS iff it is below count, its
 *   score is not NaN and score >= score_thr.  The existing rows are visited in descending score, equal scores
 *   (-0 equals +0) in ascending row index.  A visited row is kept iff no previously kept row suppresses it; row j
 *   suppresses row i iff iou(j, i) > iou_thr (strict; j the earlier, the pair computed in j's frame; bev with
 *   use_3d == 0, iou3d otherwise) and, with labels given, labels[j] == labels[i].  An invalid box that exists is
 *   kept and suppresses nothing.
 *   keep_idx int32 [N]: the kept rows in visiting order, then -1.  keep (null, or uint8 [N] with keep_dtype 0,
 *   int32 [N] with keep_dtype 1): 1 for a kept row, else 0.  keep_count: a device int32.
 *   The contract binds only inputs in which every pair the loop can compare (two existing valid rows, of equal
 *   label when labels are given) has |iou - iou_thr| > 8e-5, iou the exact value of the formulas above: the
 *   float32 evaluation is held to 1e-5 of it on the host and to 8 times the host's error on the device; nearer to
 *   the threshold than that it may fall on either side.
 *   Three launches ordered by the stream only: (1) one workgroup ranks the rows, a bitonic sort of (key, index)
 *   words in LDS; (2) a grid over the upper triangle of 64 x 64 tiles in rank order writes the suppression
 *   matrix as 64-bit words, bit b of word (r, w) = rank r suppresses rank 64 w + b (ranks after r only): the 64
 *   lanes of a wave are the 64 bits of a word; (3) one wave runs the greedy scan, lane l holding word l of the
 *   removed set, the mask rows loaded 8 rows ahead whatever the outcome of the rows before.  Every word the scan
 *   uses is rewritten by (2) before: the workspace needs no initialisation.
 *   workspace: 8-byte aligned, cmt_box_nms_workspace_bytes(N) = 16 + 4 Np + Np * Np / 8 bytes, Np = N rounded up
 *   to a multiple of 64 (-1 for N outside [0, CMT_NMS_MAX]).
 *   CMT_EINVAL: a null struct; N outside [0, CMT_NMS_MAX]; ld < 7; z_origin not 0 or 0.5; iou_thr not finite or
 *   negative; score_thr NaN; keep_dtype not 0 or 1; with N > 0 a null boxes, scores or keep_idx; a null
 *   keep_count or workspace; a misaligned pointer (4 bytes, workspace 8); workspace_bytes too small.
 *
 * cmt_box_concat.  K <= CMT_CONCAT_MAX sources, source k with boxes [n_k][ld_k], scores fp32 [n_k], labels int32
 *   [n_k], count_k null (n_k) or a device int32 clamped to [0, n_k], and with has_transform[k] a HOST float[12],
 *   row-major 3 x 4 [R|t] (Rab = transform[4a + b], ta = transform[4a + 3]).  cols in 7..16 columns are carried,
 *   every ld_k and ld_out >= cols.  Row i of source k goes to row e = n_0 + .. + n_(k-1) + i of the outputs:
 *     i < count_k: score and label copied; without a transform the columns copied bit for bit; with one
 *       x' = ((R00 * x + R01 * y) + R02 * z) + t0, y' and z' likewise with rows 1 and 2; sizes unchanged;
 *       yaw' = yaw + atan2f(R10, R00) (the angle computed once on the host in float32, no wrap);
 *       with cols >= 9: vx' = R00 * vx + R01 * vy, vy' = R10 * vx + R11 * vy; columns from 9 on copied.
 *     i >= count_k: score -inf, label -1, the cols columns 0.
 *   out_source int32 [sum n_k] = k for the whole segment, out_count (device int32) = sum n_k.  One launch, one
 *   writer per element.  cmt_box_nms drops the -inf rows through any score_thr above -inf.
 *   CMT_EINVAL: a null struct; K outside 1..CMT_CONCAT_MAX; cols outside 7..16; ld_out or an ld_k < cols; an
 *   n_k < 0; the total capacity >= 2^30; a transform that is not finite; with n_k > 0 a null boxes, scores or
 *   labels; with a total > 0 a null output; a null out_count; a misaligned (4 bytes) pointer. */
#define CMT_NMS_MAX 2048
#define CMT_CONCAT_MAX 8
typedef struct cmt_box_iou_args {
    int N, M, lda, ldb;
    int aligned, reserved;
    float z_origin, reserved_f;
    int64_t ldo;
    const void* a;
    const void* b;
    const int* n_a;
    const int* n_b;
    void* bev;
    void* iou3d;
} cmt_box_iou_args;
typedef struct cmt_box_nms_args {
    int N, ld, use_3d, keep_dtype;
    float iou_thr, score_thr, z_origin, reserved_f;
    const void* boxes;
    const void* scores;
    const int* labels;
    const int* count;
    int* keep_idx;
    void* keep;
    int* keep_count;
    void* workspace;
    int64_t workspace_bytes;
} cmt_box_nms_args;
typedef struct cmt_box_concat_args {
    int K, cols, ld_out, reserved;
    int n[CMT_CONCAT_MAX], ld[CMT_CONCAT_MAX], has_transform[CMT_CONCAT_MAX];
    float transform[CMT_CONCAT_MAX][12];
    const void* boxes[CMT_CONCAT_MAX];
    const void* scores[CMT_CONCAT_MAX];
    const int* labels[CMT_CONCAT_MAX];
    const int* count[CMT_CONCAT_MAX];
    void* out_boxes;
    void* out_scores;
    int* out_labels;
    int* out_source;
    int* out_count;
} cmt_box_concat_args;
int64_t cmt_box_iou_args_size(void);
int64_t cmt_box_nms_args_size(void);
int64_t cmt_box_concat_args_size(void);
int64_t cmt_box_nms_workspace_bytes(int N);
int cmt_box_iou(const cmt_box_iou_args* args, void* stream);
int cmt_box_nms(const cmt_box_nms_args* args, void* stream);
int cmt_box_concat(const cmt_box_concat_args* args, void* stream);

/* ---- tracking evaluation (moteval.hip; additive to ABI 25) -------------------------------------------------
 * CLEAR MOT (MOTA, MOTP, id switches, fragmentations) as the motmetrics package accumulates it, swept over
 * recall levels as the nuScenes tracking devkit does (AMOTA, AMOTP), for boxes, track ids and ground truth with
 * instance ids that already live on the device.  THIS TEXT is the contract.  It is written from the public
 * description of both packages and has NOT been compared with an installed devkit or motmetrics; the stated
 * deviations are listed at the end.
 *
 * Inputs.  Predictions: N rows of box fp32 (row stride ld_pred >= 2 floats; column 0 is the centre's x, column 1
 * its y, nothing else is read), score fp32, label, track and frame int32.  Ground truth: G rows of box (ld_gt),
 * label, frame and inst int32, the object's instance id inside its scene.  N and G are capacities: with n_pred /
 * n_gt non-null only rows below that device word (clamped to [0, capacity]) exist.  frame_tab int32 [F][2] gives
 * (scene, step) of a frame; two frames must not share a pair (not checked on the device: their rows would form one
 * frame).  A row is IGNORED when its label is outside [0, C), its frame outside [0, F), the frame's scene outside
 * [0, S) or step outside [0, Fmax), its x or y is not finite, or it fails the range test
 * sqrt(x * x + y * y) < range[label] (float64 on the float32 centre, product, sum and root rounded on their own,
 * strict: the test of cmt_det_eval_*); a prediction also when track < 0 or its score is not finite, a ground-truth
 * row also when inst is outside [0, max_gt_tracks).  The other rows are KEPT.  Instance ids of the kept ground
 * truth of one frame and class must be distinct (two rows of one instance in one frame leave the instance's
 * state, and with it IDS and FRAG, unspecified; every access stays in bounds).
 * Config: C <= 64 classes with range[c] (float64) and dist_th[c] (float32 metres), R <= 64 recall levels
 * recall[k] in (0, 1] (the caller computes r_k = min_recall + k (1 - min_recall) / (R - 1) in float64, r_0 = 1 for
 * R = 1), max_gt_tracks <= 65536.
 *
 * A CHAIN is (scene, class) in phase 1 and (scene, class, slot k) in phase 2; its number is scene * C + class,
 * resp. (scene * C + class) * R + k.  It walks step = 0 .. Fmax - 1 and keeps per instance o: m[o], the track it
 * was last matched to (-1: never), and lost[o], set when it was matched before and missed at its latest
 * appearance.  A kept prediction is ACTIVE in a chain iff score >= the chain's threshold (float32, inclusive;
 * phase 1: every kept prediction is active).  At a step the chain sees the kept ground truth i = 0 .. n_gt - 1 of
 * its (frame, class) in row order and the active predictions j = 0 .. n_pred - 1 in row order, and does:
 *  1. d_ij = sqrtf(fl32(fl32(dx * dx) + fl32(dy * dy))), dx, dy the float32 centre differences: every operation is
 *     an IEEE single operation rounded on its own (the file is built with -ffp-contract=off; hipcc's default
 *     float32 sqrt is correctly rounded).  A pair is ADMISSIBLE iff d_ij < dist_th[class] (strict; a non-finite d
 *     fails).
 *  2. Sticky pass, i ascending: if m[o_i] >= 0 and an active, not yet taken j has track_j == m[o_i] and (i, j) is
 *     admissible, the lowest such j is matched to i and both are taken.
 *  3. Assignment: cost[i][j] = d_ij if (i, j) is admissible and neither is taken, else CMT_MOT_BIG; the matrix
 *     [n_gt][n_pred] (row stride ld) and its descriptor (offset, n_gt, n_pred, ld) go through cmt_lsap (Nq = n_gt,
 *     ngt = n_pred) unchanged.  A pair counts iff match_g[i] == j, match_q[j] == i and cost[i][j] < CMT_MOT_BIG.
 *     The optimum minimises the sum of distances over the largest number of admissible pairs; where it is not
 *     unique cmt_lsap's tie rule (its header text) decides.
 *  4. Accounting, i ascending.  Matched to a prediction of track h at distance d:  TP += 1; dist_sum += d (a
 *     float64 sum of the float32 d, in this order); IDS += 1 if m[o] >= 0 and m[o] != h; FRAG += 1 if lost[o]; then
 *     m[o] = h, lost[o] = 0.  Unmatched: FN += 1; lost[o] = (m[o] >= 0).  FP += n_pred - (matches of the step),
 *     NPRED += n_pred.  The six counters are int64 in the order TP, FP, FN, IDS, FRAG, NPRED.
 * Phase 1 also writes tp_score[g] for every ground-truth row g: the score of its matched prediction, a quiet NaN
 * for an unmatched or ignored row; and tp_key[g] = class << 32 | ~ord(score) (INT64_MAX where tp_score is NaN; ord:
 * the order-preserving uint32 of a float, -0 as +0), which the caller sorts ascending: per class the true-positive
 * scores in descending order.
 * Thresholds.  npos[c] = the kept ground truth of class c.  need_k = max(1, ceil(recall[k] * npos)), the product
 * in float64.  thr[c][k] = the need_k-th (1-based) of the class's descending true-positive scores; with fewer true
 * positives, or npos = 0, the slot is NOT ACHIEVED and thr is a quiet NaN.  A chain of a slot not achieved does
 * nothing: all its counters are 0.
 * Summary.  Per (class, slot) the chains' counters are added over the scenes in ascending scene order (integers;
 * dist_sum as a float64 sum in that order) into counters[C][R][6] and dist_sum[C][R]; likewise phase 1 into
 * counters1[C][6] and dist_sum1[C].  metrics[C][R][4] = recall, MOTA, MOTP, MOTAR in float64, every operation
 * rounded on its own, with n = npos, e = IDS + FP + FN (int64):
 *   recall = TP / n;  MOTA = 1 - e / n;  MOTP = dist_sum / TP (dist_th if TP = 0);
 *   MOTAR = max(0, 1 - (e - (1 - recall) * n) / (recall * n)), 0 if TP = 0.
 * A slot not achieved has recall = MOTA = MOTAR = 0 and MOTP = dist_th (its counters are 0).  class_sum[C][12]
 * float64: AMOTA (the mean of MOTAR over all R slots, a serial sum in slot order divided by R), AMOTP (the same
 * mean of MOTP), best (the achieved slot of highest MOTA, the lowest k on a tie; -1 if none is achieved), then
 * that slot's MOTA, MOTP, recall, TP, FP, FN, IDS, FRAG and threshold (NaN if best = -1).  A class with npos = 0
 * has NaN in all of metrics and class_sum but best = -1.
 *
 * Calls, all stream-ordered, one args struct:
 *   cmt_mot_eval_keys        key_pred[N], key_gt[G] int64 = ((scene * Fmax + step) << 6 | class) << 32 | row, INT64_MAX
 *                            for an ignored row; tp_score / tp_key of the ignored ground-truth rows.
 *   the caller sorts both key arrays ascending (sk_pred, sk_gt): the kept rows of one (frame, class) become one
 *   contiguous run in row order, found by binary search.
 *   cmt_mot_eval_runs        npos[C] and run_max[2][CMT_MOT_RUN_PARTS] int32: the longest run of ground truth ([0][s]) and
 *                            of predictions ([1][s]) among the runs that end in slice s of the sorted keys (slice s holds
 *                            the tiles of 256 keys whose number is s modulo CMT_MOT_RUN_PARTS).  The caller reads them
 *                            once and passes Gmax >= the largest of run_max[0], Hmax >= the largest of run_max[1].
 *   per phase, per block of chains [chain0, chain0 + nchains), per step 0 .. Fmax - 1 in order:
 *     cmt_mot_eval_cost      one wave per chain: active predictions compacted in row order into cols[nchains][Hmax]
 *                            (prediction rows), the sticky pass into smatch[nchains][Gmax] (column or -1), cost
 *                            [nchains][Gmax][Hmax] and desc[nchains][4] = (chain * Gmax * Hmax, n_gt, n_pred, Hmax);
 *                            at step 0 also m = -1, lost = 0 for the block's state_m [nchains][max_gt_tracks] int32
 *                            and state_lost (uint8).  Runs longer than Gmax / Hmax are cut there.
 *     cmt_lsap               P = nchains, max_nq = max(Gmax, 1), max_ngt = max(Hmax, 1), match_g rows of Gmax,
 *                            match_q rows of Hmax.
 *     cmt_mot_eval_update    one wave per chain: the accounting into chain_cnt[chains of the phase][6] int64 and
 *                            chain_dist (float64) of the chain's own number (step 0 starts from 0, so nothing
 *                            needs a memset), the state, and in phase 1 tp_score / tp_key.
 *   The blocks of a phase cover its chains once each; the result does not depend on the split.
 *   cmt_mot_eval_thresholds  after phase 1 and the caller's ascending sort of tp_key (sk_tp, si_tp): thr[C][R].
 *   cmt_mot_eval_summary     after phase 2: the outputs of "Summary" from chain_cnt1 / chain_dist1 [S * C] and
 *                            chain_cnt2 / chain_dist2 [S * C * R].
 * Every output element has exactly one writer, there are no atomics, two runs are bitwise equal.  Counts and ids
 * read from device memory (n_pred, n_gt, desc, inst, the match tables, si_tp) are clamped or range-checked before
 * they index anything.
 * CMT_EINVAL before any device work: a null struct; N or G outside [0, 2^31); F, S, Fmax, C, R or max_gt_tracks
 * < 1; S * Fmax > 2^24; ld_pred or ld_gt < 2; a range or dist_th that is not finite and positive; a recall level
 * outside (0, 1]; phase not 1 or 2; step outside [0, Fmax); chain0 < 0, nchains < 1 or chain0 + nchains above
 * the phase's chains; Gmax or Hmax < 0; a null or misaligned pointer that the call uses (the row arrays only with
 * N resp. G > 0).  CMT_ENOTSUP: C > 64; R > 64; max_gt_tracks > 65536; nchains > 65535; Gmax > 512; Hmax > 2048
 * (the last three are cmt_lsap's own limits).
 * Deviations from the devkit: the thresholds are order statistics of the true-positive scores (the devkit
 * interpolates between them with numpy.interp); MOTAR uses the achieved recall; there is no max_switch_time; the
 * devkit's track interpolation, its TID / LGD / FAF and the per-scene breakdown are not computed. */
#define CMT_MOT_MAX_CLASSES 64
#define CMT_MOT_MAX_THRESHOLDS 64
#define CMT_MOT_MAX_GT_TRACKS 65536
#define CMT_MOT_MAX_GT 512
#define CMT_MOT_MAX_PRED 2048
#define CMT_MOT_MAX_CHAINS 65535
#define CMT_MOT_RUN_PARTS 64
#define CMT_MOT_BIG 1.0e6f
typedef struct cmt_mot_eval_args {
    int64_t N, G;                                  /* capacities (rows) */
    int F, S, Fmax, C, R, ld_pred, ld_gt, max_gt_tracks;
    int phase, step, chain0, nchains, Gmax, Hmax;  /* cost / update only */
    double range[CMT_MOT_MAX_CLASSES], recall[CMT_MOT_MAX_THRESHOLDS];
    float dist_th[CMT_MOT_MAX_CLASSES];
    const void *pred_box, *pred_score, *pred_label, *pred_track, *pred_frame;
    const void *gt_box, *gt_label, *gt_frame, *gt_inst;
    const int *n_pred, *n_gt;                      /* device words, or null: all rows */
    const void* frame_tab;                         /* int32 [F][2] */
    void *key_pred, *key_gt;                       /* int64 [N], [G]: written by cmt_mot_eval_keys */
    const void *sk_pred, *sk_gt;                   /* int64: the sorted keys */
    void *npos, *run_max;                          /* int32 [C], [2][CMT_MOT_RUN_PARTS]: written by cmt_mot_eval_runs */
    void *tp_score, *tp_key;                       /* fp32 [G], int64 [G] */
    const void *sk_tp, *si_tp;                     /* int64 [G]: tp_key sorted, and the sort's indices */
    void* thr;                                     /* fp32 [C][R] */
    void *chain_cnt1, *chain_dist1, *chain_cnt2, *chain_dist2;
    void *state_m, *state_lost, *cost, *desc, *cols, *smatch;   /* the block's workspace */
    const int *match_q, *match_g;                  /* cmt_lsap's tables, rows of Hmax and Gmax */
    void *counters, *dist_sum, *metrics, *class_sum, *counters1, *dist_sum1;
} cmt_mot_eval_args;
int64_t cmt_mot_eval_args_size(void);
int cmt_mot_eval_keys(const cmt_mot_eval_args* args, void* stream);
int cmt_mot_eval_runs(const cmt_mot_eval_args* args, void* stream);
int cmt_mot_eval_cost(const cmt_mot_eval_args* args, void* stream);
int cmt_mot_eval_update(const cmt_mot_eval_args* args, void* stream);
int cmt_mot_eval_thresholds(const cmt_mot_eval_args* args, void* stream);
int cmt_mot_eval_summary(const cmt_mot_eval_args* args, void* stream);

/* ---- result pictures: top view and camera overlays (render.hip; additive to ABI 25) --------------------------
 * Points, line segments, box wire frames and decimal numbers drawn into pictures on the device, from buffers that
 * already live there.  THIS TEXT is the contract.  Every sum, difference, product and quotient below is an IEEE
 * single operation rounded on its own (none is fused), in the order the parentheses give.  Caller-owned buffers,
 * stream-ordered, no allocation, no host read: graph-capturable.  Every CMT_EINVAL below is returned before any
 * device work.
 *
 * THE KEY PLANE.  A picture in progress is a uint64 [V][H][W] plane that the caller clears to 0.  Every drawing
 * call does nothing but atomic maxima (64-bit vector atomics on global memory) on it with the key
 *   key = layer << 56 | order << 24 | rgb        layer 8 bits, order 32 bits, rgb 24 bits (r << 16 | g << 8 | b)
 * Maximum is commutative and idempotent: the finished plane does not depend on the order of the launches, of the
 * waves or of the writers of a pixel, so it is bitwise repeatable with no ordering machinery.  Key 0 is "empty"; no
 * call below writes it (every order below is non-zero).  layer is chosen per call, 0..255; a higher layer covers a
 * lower one, within a layer the higher order wins, then the higher rgb.  Colours are uint32 words of which only the
 * low 24 bits are used.
 *   okey(f), the order-preserving map of a float to uint32: bits ^ 0x80000000 with the sign bit clear, ~bits
 *   otherwise.  okey(-0) + 1 == okey(+0); a finite f gives neither 0 nor 0xFFFFFFFF.
 *
 * VIEWS.  view[v], v < V <= CMT_RENDER_MAX_VIEWS, is a HOST row-major 4 x 4 float matrix m.  Row r of a scene
 * position (x, y, z):  R_r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3].  The pixel coordinates are
 * u = R_0 / R_3, v = R_1 / R_3, the depth is d = R_2.  A camera passes its lidar2img with row 3 set to row 2 (the
 * depth row, by which lidar2img divides), the top view an orthographic matrix (row 3 = 0 0 0 1, row 2 = 0 0 1 0).
 * A position is BEHIND the view unless R_3 >= near (near: 0.1 for a camera, anything below 1 for the top view).
 * Pixel (X, Y) of view v is plane[(v * H + Y) * W + X]; it covers X <= u < X + 1, Y <= v < Y + 1.  Every test on u
 * and v is made on the floats before a conversion to int: a NaN or an infinity never reaches a cast.
 *
 * cmt_render_points.  points fp32 [N][ld], ld >= 3, columns x y z first; n null (N) or a device int32 clamped to
 *   [0, N].  For a row below n and every view: the row is skipped if x, y or z is not finite (the NaN padding of
 *   cmt_pts_prepare goes in as it is), if it is behind the view, if d is not finite or unless 0 <= u < W and
 *   0 <= v < H.  X = floor(u), Y = floor(v).
 *   c = the row's column color_col (3 <= .. < ld; or 0..2), or d with color_col == -1;
 *   t = ((c - lo) * inv_span) * 255;  index = 255 if t >= 255, floor(t) if 0 <= t < 255, else 0 (a NaN gives 0);
 *   rgb = lut[index] (a device uint32 [256]);  order = okey(d), or ~okey(d) with near_wins != 0 (the top view leaves
 *   it clear: the highest point wins; a camera sets it: the nearest wins).
 *   The key goes to every pixel (X + i, Y + j), |i|, |j| <= radius (0..2), that lies inside the picture.
 *   One lane per row, grid-stride, one launch for all V views.
 *
 * THE SEGMENT, shared by cmt_render_segments, cmt_render_boxes (one device function).  Ends a and b, a view:
 *   (1) [not planar]  the segment is dropped if a coordinate is not finite.  A_r, B_r: the rows of a and b, r = 0..3;
 *       dropped if one of the eight is not finite.  ina = A_3 >= near, inb = B_3 >= near; dropped if neither.  If
 *       exactly one holds: t = (near - A_3) / (B_3 - A_3), C_r = A_r + t * (B_r - A_r) for r = 0, 1, and the end that
 *       is behind is replaced by (C_0, C_1, near).  Then ua = A_0 / A_3, va = A_1 / A_3, ub = B_0 / B_3,
 *       vb = B_1 / B_3.
 *       [planar]  ua, va, ub, vb are the given coordinates.
 *       Dropped unless ua, va, ub, vb, dx = ub - ua and dy = vb - va are all finite.
 *   (2) Liang-Barsky against the picture grown by one pixel, xmin = ymin = -1, xmax = W + 1, ymax = H + 1 (as floats).
 *       t0 = 0, t1 = 1; for (p, q) in (-dx, ua - xmin), (dx, xmax - ua), (-dy, va - ymin), (dy, ymax - va), in that
 *       order:  if p == 0: dropped if q < 0, else the next pair;  r = q / p;  if p < 0: dropped if r > t1, and
 *       t0 = r if r > t0;  if p > 0: dropped if r < t0, and t1 = r if r < t1.
 *       (xa, ya) = (ua + t0 * dx, va + t0 * dy) if t0 > 0, else (ua, va);
 *       (xb, yb) = (ua + t1 * dx, va + t1 * dy) if t1 < 1, else (ub, vb).
 *   (3) X0 = floor(xa) clamped to [-2, W + 2], Y0 = floor(ya) clamped to [-2, H + 2] (the clamps on the floats), X1
 *       and Y1 likewise from (xb, yb).
 *   (4) THE INTEGER WALK.  dX = X1 - X0, dY = Y1 - Y0, n = max(|dX|, |dY|).  For k = 0..n the pixel is
 *       (X0 + floordiv(2 * dX * k + n, 2 * n), Y0 + floordiv(2 * dY * k + n, 2 * n)), floordiv rounding towards minus
 *       infinity; n == 0 draws the one pixel (X0, Y0).  The walk from b to a visits the same pixels.
 *       With thickness t in 1..3 every walk pixel (X, Y) stands for the t x t square X + i, Y + j with
 *       -((t - 1) / 2) <= i, j <= t / 2 (integer divisions).  Pixels outside the picture are not written.
 *   One wave per (segment, view), the lanes across k.
 *
 * cmt_render_segments.  p0, p1 fp32 [S][3] scene positions, or with planar != 0 [S][2] pixel coordinates (no view
 *   is applied; the segment is drawn into all V pictures); rgb uint32 [S]; rank int32 [S] or null (the segment
 *   index); n null (S) or a device int32 clamped to [0, S].  order = 0xFFFFFFFF - max(rank, 0): the lower rank
 *   lies on top.
 *
 * cmt_render_boxes.  Rows fp32 [M][ld], ld >= 7, z_origin in {0, 0.5}, validity and derived values hx, hy, s, c,
 *   bot, top exactly as cmt_box_iou (one sinf / cosf pair per box).  A row draws nothing if it is invalid, at or
 *   beyond count (null: M; a device int32 clamped to [0, M]), or, with scores given, unless score > score_thr.
 *   Corners k = 0..3 with (sx, sy) = (-,-), (-,+), (+,+), (+,-), cmt_box_iou's order:
 *     lx = sx * hx, ly = sy * hy,  X_k = (lx * c - ly * s) + x,  Y_k = (lx * s + ly * c) + y;
 *   corner k is (X_k, Y_k, bot), corner k + 4 is (X_k, Y_k, top).  Thirteen segments, each from the first corner named
 *   to the second: (k, (k + 1) mod 4), (k + 4, (k + 1) mod 4 + 4), (k, k + 4) for k = 0..3, and the heading mark from
 *   (x, y, top) to (hx * c + x, hx * s + y, top).  rgb = class_rgb[label] with labels and class_rgb given and
 *   0 <= label < ncls, else rgb_default.  order = 0xFFFFFFFF - row index: the better-scoring rows of a decoded frame
 *   lie on top.  One wave per (box, view).
 *
 * cmt_render_digits.  values int32 [M] (a negative value draws nothing), anchors fp32 [M][3] scene positions or,
 *   with planar != 0, [M][2] pixel coordinates; rgb uint32 [M] or null (rgb_one); rank as for segments; scale 1..4.
 *   The anchor is projected as a point is; it is dropped if it is behind the view, or unless -65536 <= u < 65536 and
 *   -65536 <= v < 65536.  X0 = floor(u), Y0 = floor(v) is the top left pixel of the first digit.  The decimal digits,
 *   most significant first, digit j at cell column 6 * j (one column of space).  Cell (cx, cy), cx = 0..4 from the
 *   left, cy = 0..6 from the top, of digit g is set iff bit (4 - cx) of font[g][cy] is set; a set cell covers the
 *   scale x scale pixels (X0 + (6 * j + cx) * scale + i, Y0 + cy * scale + l), 0 <= i, l < scale, inside the picture.
 *   font[10][7] = {0x0E,0x11,0x13,0x15,0x19,0x11,0x0E}, {0x04,0x0C,0x04,0x04,0x04,0x04,0x0E},
 *     {0x0E,0x11,0x01,0x02,0x04,0x08,0x1F}, {0x1F,0x02,0x04,0x02,0x01,0x11,0x0E}, {0x02,0x06,0x0A,0x12,0x1F,0x02,0x02},
 *     {0x1F,0x10,0x1E,0x01,0x01,0x11,0x0E}, {0x06,0x08,0x10,0x1E,0x11,0x11,0x0E}, {0x1F,0x01,0x02,0x04,0x08,0x08,0x08},
 *     {0x0E,0x11,0x11,0x0E,0x11,0x11,0x0E}, {0x0E,0x11,0x11,0x0F,0x01,0x02,0x0C}.
 *   One wave per (value, view), the lanes across (digit, cell).
 *
 * cmt_render_resolve.  plane -> out uint8 [V][H][W][3] (r, g, b).  A pixel with key 0 takes the pixel of
 *   src uint8 [V][H][W][3] if src is given, else background; any other pixel takes the key's rgb.  out == src is
 *   allowed (a thread reads and writes its own pixel only); any other overlap is not.
 *
 * Limits and CMT_EINVAL, all calls: a null struct; V outside 1..CMT_RENDER_MAX_VIEWS; H or W outside 1..4096; layer
 *   outside 0..255; near or a used view entry not finite; a null or misaligned plane (8 bytes); another misaligned
 *   pointer (4 bytes; the uint8 pictures 1).  points: N outside [0, 2^31); ld < 3; color_col outside -1..ld-1;
 *   radius outside 0..2; lo or inv_span not finite; with N > 0 a null points or lut.  segments: S outside
 *   [0, CMT_RENDER_MAX_ITEMS); thickness outside 1..3; with S > 0 a null p0, p1 or rgb.  boxes: M outside
 *   [0, CMT_RENDER_MAX_ITEMS); ld < 7; z_origin not 0 or 0.5; thickness outside 1..3; score_thr NaN; ncls < 0; with
 *   M > 0 a null boxes.  digits: M outside [0, CMT_RENDER_MAX_ITEMS); scale outside 1..4; with M > 0 a null values or
 *   anchors.  resolve: a null out.  A count of 0 is a valid call that launches nothing. */
#define CMT_RENDER_MAX_VIEWS 8
#define CMT_RENDER_MAX_SIZE 4096
#define CMT_RENDER_MAX_ITEMS 1048576
typedef struct cmt_render_target {
    int V, H, W, layer;
    float near, reserved_f;
    float view[CMT_RENDER_MAX_VIEWS][16];
    void* plane;                              /* uint64 [V][H][W] */
} cmt_render_target;
typedef struct cmt_render_points_args {
    cmt_render_target t;
    int N, ld, radius, near_wins, color_col, reserved;
    float lo, inv_span;
    const void* points;
    const int* n;
    const void* lut;                          /* uint32 [256] */
} cmt_render_points_args;
typedef struct cmt_render_segments_args {
    cmt_render_target t;
    int S, planar, thickness, reserved;
    const void* p0;
    const void* p1;
    const void* rgb;                          /* uint32 [S] */
    const int* rank;
    const int* n;
} cmt_render_segments_args;
typedef struct cmt_render_boxes_args {
    cmt_render_target t;
    int M, ld, thickness, ncls;
    float z_origin, score_thr;
    uint32_t rgb_default, reserved;
    const void* boxes;
    const int* count;
    const int* labels;
    const void* scores;
    const void* class_rgb;                    /* uint32 [ncls] */
} cmt_render_boxes_args;
typedef struct cmt_render_digits_args {
    cmt_render_target t;
    int M, planar, scale, reserved;
    uint32_t rgb_one, reserved_u;
    const void* values;                       /* int32 [M] */
    const void* anchors;
    const void* rgb;                          /* uint32 [M] or null */
    const int* rank;
} cmt_render_digits_args;
typedef struct cmt_render_resolve_args {
    int V, H, W, reserved;
    uint32_t background, reserved_u;
    const void* plane;
    const void* src;                          /* uint8 [V][H][W][3] or null */
    void* out;                                /* uint8 [V][H][W][3] */
} cmt_render_resolve_args;
int64_t cmt_render_points_args_size(void);
int64_t cmt_render_segments_args_size(void);
int64_t cmt_render_boxes_args_size(void);
int64_t cmt_render_digits_args_size(void);
int64_t cmt_render_resolve_args_size(void);
int cmt_render_points(const cmt_render_points_args* args, void* stream);
int cmt_render_segments(const cmt_render_segments_args* args, void* stream);
int cmt_render_boxes(const cmt_render_boxes_args* args, void* stream);
int cmt_render_digits(const cmt_render_digits_args* args, void* stream);
int cmt_render_resolve(const cmt_render_resolve_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMT_HIP_H */
