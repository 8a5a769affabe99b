// Image backbone kernels (VoVNet-eSE, the reference's img_backbone), declared in include/cmt_hip.h
// (cmt_img_* and cmt_img_*_f16):
//   img_stem_kernel      3 x 3 / stride 2 / pad 1 conv from the fp32 NCHW image to rows
//   img_conv3x3_kernel   3 x 3 / pad 1 conv of stride 1 or 2, rows to rows, any Cout % 32 <= 256
//   img_concat_kernel    1 x 1 conv over up to 8 row sources (the OSA aggregation without a
//                        concatenated map), with the eSE pool's per-tile column sums
//   img_gate_kernel      eSE gate: hsigmoid(fc(mean)) from the per-tile sums, fp32 FMA
//   img_apply_kernel     x * gate (+ identity) on rows
//   img_pool_kernel      3 x 3 / stride 2 / ceil-mode / no-pad max on rows
// Every kernel but the gate is one body over an arithmetic policy: X3 (cmt_img_*: CMT_F16P pair rows, three
// f16 MFMA passes lo*Whi + hi*Wlo + hi*Whi per 16-k step) or F16 (cmt_img_*_f16, opt-in: plain fp16 rows, W
// rounded once to fp16, one MFMA per step).  The conv and the concat are output-stationary: a wave owns 32
// output rows x all of the workgroup's columns (NB accumulators of 32 columns), gathers an A fragment once
// per 16-channel step straight into the MFMA operand layout (lane (r, h): row r, channels 8h .. 8h+7) and
// uses it for every column block.  W goes through LDS in chunks of the policy's KC, staged once for the four
// waves, double-buffered, one barrier per chunk.  fp32 accumulation in fixed K order: tap-major
// (source-major), channels ascending.  No atomics on the data path (one writer per element), no call
// synchronises with the host.
#include "cmt_common.h"

namespace {

constexpr int IMG_TM = 128;     // output rows per workgroup (4 waves x 32)
constexpr int IMG_WROW = 64;    // 16-bit words per LDS row of a W chunk (X3: hi 32 | lo 32, F16: 64 k)
constexpr int IMG_STEM_K = 32;  // the stem's K = 9 Cin <= 27, zero-padded: two 16-k steps
constexpr int IMG_CAT_NB = 4;   // concat: 32-column blocks per workgroup (128 output channels)
constexpr int IMG_GATE_OB = 16; // gate: outputs per workgroup (4 per wave)

// Piece i of thread t of a W chunk: row (t >> 3) + 32 i, 16 bytes sub = t & 7 of the row's 128.  In LDS
// the piece index is XORed with (row >> 1) % 8: two rows fill one 256-byte bank row, so 16 consecutive
// rows at one logical piece (a ds_read_b128 group) fall on 16 distinct 16-byte slots.
template <int NB>
__device__ __forceinline__ void w_store(pair_t* buf, const pair8_t (&q)[NB], int t) {
    const int row = t >> 3;
    pair_t* dst = buf + row * IMG_WROW + (((t & 7) ^ ((row >> 1) & 7)) * 8);
#pragma unroll
    for (int i = 0; i < NB; ++i) *(pair8_t*)(dst + 32 * i * IMG_WROW) = q[i];
}

// ---- the arithmetic policies: only what differs between the two row formats ------------------------------------
// A lane's A fragments of one chunk are pair8_t a[4] (X3: lo of step j at a[j], hi at a[2 + j]; F16: step j at
// a[j]): a plain array that the kernels copy element by element, and lo first, because a step's first MFMA reads
// lo; both spellings are load-bearing for the schedule (profiles/img_refactor_isa.txt).
// a_load: KC channels from c of a row of width C (xr already at the lane's 8 h), zero where the row is padding.
// a_set: element jj of step j from an fp32 value (the stem).  w_load: rows [n0, n0 + 32 NB) x one chunk from
// k offset kb of W into the pieces w_store takes.  mma: one 16-k step j against 8 words of a W row (b: the step's
// piece, b_lo: the piece KC further).  store: one output value, returned as stored.  Raw8 / load8 / value / take
// / store8 / write8: 8 channels of apply and pool.

// CMT_F16P pair rows [rows][2][C] and the [N][2][Ktot] pair image of W; a chunk is hi | lo of 32 k.
struct X3 {
    static constexpr int KC = 32, STEPS = 2;
    static constexpr int WORDS = 2;          // 16-bit words per element
    static constexpr bool HALF = false;      // every width is a multiple of KC
    static constexpr bool LDY8 = false;      // host: stem, conv and concat take any ldy
    static __device__ __forceinline__ int chunks(int C) { return C / KC; }
    static __device__ __forceinline__ void a_load(pair8_t (&a)[4], const pair_t* xr, bool ok, int c, int C, bool) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            a[j] = zero8();
            a[2 + j] = zero8();
            if (ok) {
                a[2 + j] = *(const pair8_t*)(xr + c + 16 * j);
                a[j] = *(const pair8_t*)(xr + C + c + 16 * j);
            }
        }
    }
    static __device__ __forceinline__ void a_set(pair8_t (&a)[4], int j, int jj, float v) {
        pair_t hi, lo;
        split_pair(v, hi, lo);
        a[2 + j][jj] = hi;
        a[j][jj] = lo;
    }
    // the hi plane and the lo plane lie Ktot apart (hi: sub < 4)
    template <int NB>
    static __device__ __forceinline__ void w_load(pair8_t (&q)[NB], const pair_t* Wt, int64_t ldw, int Ktot, int n0, int kb,
                                                  bool, int t) {
        const int sub = t & 7;
        const pair_t* src = Wt + (int64_t)(n0 + (t >> 3)) * ldw + (sub >> 2) * Ktot + kb + 8 * (sub & 3);
#pragma unroll
        for (int i = 0; i < NB; ++i) q[i] = *(const pair8_t*)(src + (int64_t)(32 * i) * ldw);
    }
    static __device__ __forceinline__ f32x16 mma(const pair8_t (&a)[4], int j, const pair_t* b, const pair_t* b_lo, f32x16 c) {
        return mma3(a[2 + j], a[j], *(const pair8_t*)b, *(const pair8_t*)b_lo, c);
    }
    static __device__ __forceinline__ float store(pair_t* row, int C, int col, float v) {
        pair_t hi, lo;
        split_pair(v, hi, lo);
        row[col] = hi;
        row[C + col] = lo;
        return (float)hi + (float)lo;
    }
    struct Raw8 {
        pair8_t hi, lo;
        float v[8];
    };
    static __device__ __forceinline__ Raw8 load8(const pair_t* x, int C) {
        Raw8 q;
        q.hi = *(const pair8_t*)x;
        q.lo = *(const pair8_t*)(x + C);
#pragma unroll
        for (int j = 0; j < 8; ++j) q.v[j] = (float)q.hi[j] + (float)q.lo[j];
        return q;
    }
    static __device__ __forceinline__ float value(const Raw8& q, int j) { return q.v[j]; }
    static __device__ __forceinline__ void take(Raw8& best, const Raw8& q, int j) {
        best.v[j] = q.v[j];
        best.hi[j] = q.hi[j];
        best.lo[j] = q.lo[j];
    }
    static __device__ __forceinline__ void store8(pair_t* y, int C, const Raw8& q) {
        *(pair8_t*)y = q.hi;
        *(pair8_t*)(y + C) = q.lo;
    }
    static __device__ __forceinline__ void write8(pair_t* row, int C, int c, const float* v) { store_pair8(row, C, c, v); }
};

// Plain fp16 rows [rows][C] and W rows [N][ldw]; a chunk is 64 k, so it carries four MFMA steps per
// accumulator and the barrier, staging and gather cost per MFMA stays at 3/4 of X3's instead of tripling.
// A width with C % 64 == 32 ends in a half chunk (32 k: pieces 4 .. 7 of the LDS row are neither loaded nor
// read).
struct F16 {
    static constexpr int KC = 64, STEPS = 4;
    static constexpr int WORDS = 1;
    static constexpr bool HALF = true;
    static constexpr bool LDY8 = true;
    static __device__ __forceinline__ int chunks(int C) { return (C + KC - 1) / KC; }
    static __device__ __forceinline__ void a_load(pair8_t (&a)[4], const f16_t* xr, bool ok, int c, int, bool half) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = zero8();
            if (ok && !(half && j >= 2)) a[j] = *(const pair8_t*)(xr + c + 16 * j);
        }
    }
    static __device__ __forceinline__ void a_set(pair8_t (&a)[4], int j, int jj, float v) { a[j][jj] = (f16_t)v; }
    // a half chunk has pieces 0 .. 3 only (the others would lie in the next tap or past the row's end) and
    // leaves the registers as they are
    template <int NB>
    static __device__ __forceinline__ void w_load(pair8_t (&q)[NB], const f16_t* Wt, int64_t ldw, int, int n0, int kb,
                                                  bool half, int t) {
        const int sub = t & 7;
        if (half && sub >= 4) return;
        const f16_t* src = Wt + (int64_t)(n0 + (t >> 3)) * ldw + kb + 8 * sub;
#pragma unroll
        for (int i = 0; i < NB; ++i) q[i] = *(const pair8_t*)(src + (int64_t)(32 * i) * ldw);
    }
    static __device__ __forceinline__ f32x16 mma(const pair8_t (&a)[4], int j, const f16_t* b, const f16_t*, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a[j], *(const pair8_t*)b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float store(f16_t* row, int, int col, float v) {
        const f16_t y = (f16_t)v;
        row[col] = y;
        return (float)y;
    }
    struct Raw8 {
        pair8_t x;
    };
    static __device__ __forceinline__ Raw8 load8(const f16_t* x, int) { return Raw8{*(const pair8_t*)x}; }
    static __device__ __forceinline__ float value(const Raw8& q, int j) { return (float)q.x[j]; }
    static __device__ __forceinline__ void take(Raw8& best, const Raw8& q, int j) { best.x[j] = q.x[j]; }
    static __device__ __forceinline__ void store8(f16_t* y, int, const Raw8& q) { *(pair8_t*)y = q.x; }
    static __device__ __forceinline__ void write8(f16_t* row, int, int c, const float* v) {
        pair8_t y;
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = (f16_t)v[j];
        *(pair8_t*)(row + c) = y;
    }
};

// The conv's occupancy bound: the F16 kernels keep their accumulators in VGPRs and are held to 4 / 3 / 2 waves
// per SIMD; the X3 kernels have no bound and keep theirs in AGPRs (profiles/img_backbone_f16.txt, sessions A to C).
#define IMG_CONV_BOUNDS(P, NB) __launch_bounds__(256, P::HALF ? (NB >= 5 ? 2 : (NB >= 3 ? 3 : 4)) : 1)

// One chunk of the wave's 32 rows against the staged chunk: fragment f of step j holds row 32 f + r,
// k = 16 j + 8 h .. + 7, piece 2 j + h of the row (X3: the lo piece 4 further)
template <class P, int NB>
__device__ __forceinline__ void mma_chunk(const pair_t* buf, const pair8_t (&a)[4], f32x16 (&acc)[NB], bool half, int r, int h) {
    const int swz = (r >> 1) & 7;
#pragma unroll
    for (int j = 0; j < P::STEPS; ++j) {
        if (j >= 2 && half) break;   // workgroup-uniform
#pragma unroll
        for (int f = 0; f < NB; ++f) {
            const pair_t* row = buf + (32 * f + r) * IMG_WROW;
            acc[f] = P::mma(a, j, row + (((2 * j + h) ^ swz) * 8), row + (((4 + 2 * j + h) ^ swz) * 8), acc[f]);
        }
    }
}

// One workgroup: 128 output rows (4 waves x 32, row -> (b, yo, xo) decoded once; a tile may straddle a
// map-row end or an image boundary) x 32 NB columns from blockIdx.y * 32 NB: all Cout where the rows alone
// fill the device, a divisor of Cout / 32 per workgroup on small maps (img_conv3x3 picks; an output's sum
// has the same order either way).  The chunk sequence is tap-major, P::chunks(Cin) chunks per tap (F16: the
// last a half chunk where Cin % 64 == 32); chunk i + 1's W pieces and A fragments are loaded while chunk i's
// MFMAs run, the pieces are written to the other LDS buffer after them.  A tap that is padding for all 32
// rows of a wave costs that wave no A load and no MFMA (ballot); a wave past the last row still stages W and
// takes part in the barriers.
template <class P, int NB>
__global__ IMG_CONV_BOUNDS(P, NB) void img_conv3x3_kernel(cmt_img_conv_args a, int Ho, int Wo, int M) {
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
    const int cpt = P::chunks(Cin), nchunks = 9 * cpt;
    const bool odd = P::HALF && (Cin % P::KC) != 0;   // the last chunk of every tap is a half chunk
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

    pair8_t wq[NB], av[4], nv[4];
    if constexpr (P::HALF) {   // a half chunk leaves pieces 4 .. 7 unloaded
#pragma unroll
        for (int i = 0; i < NB; ++i) wq[i] = zero8();
    }
    bool half = odd && cpt == 1;
    P::template w_load<NB>(wq, Wt, a.ldw, Ktot, n0, 0, half, t);
    w_store<NB>(s_w[0], wq, t);
    int tap = 0, cc = 0;
    bool ok;
    const pair_t* xr = tap_src(0, ok);
    bool any = __ballot(ok) != 0;
    P::a_load(av, xr, ok, 0, Cin, half);
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
        const pair_t* nxr = xr;
        if (more) {
            P::template w_load<NB>(wq, Wt, a.ldw, Ktot, n0, ntap * Cin + P::KC * ncc, nhalf, t);
            if (ncc == 0) {
                nxr = tap_src(ntap, nok);
                nany = __ballot(nok) != 0;
            }
            P::a_load(nv, nxr, nok, P::KC * ncc, Cin, nhalf);
        }
        if (any) mma_chunk<P, NB>(s_w[it & 1], av, acc, half, r, h);   // wave-uniform
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
            P::store(Y + (int64_t)row * a.ldy, a.Cout, col, v);
        }
    }
    raise_range_flag(a.range_flag, bad);
}

// One workgroup: 128 pixels of one image (grid z) x 128 output channels (grid y); the chunk sequence
// runs source by source, P::chunks(C_s) chunks each, at k offset off_s of W.  The rest as the conv above.
// part: every wave sums its rows' values as stored per column in row order, the two lane halves are
// added, the four waves' sums meet in LDS and are added in wave order: one fixed order per tile.
template <class P>
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

    pair8_t wq[NB], av[4], nv[4];
    if constexpr (P::HALF) {
#pragma unroll
        for (int i = 0; i < NB; ++i) wq[i] = zero8();
    }
    int src = 0, cc = 0, off = 0, Cs = a.C[0];
    bool half = P::HALF && Cs < P::KC;
    P::template w_load<NB>(wq, Wt, a.ldw, Ktot, n0, 0, half, t);
    w_store<NB>(s_w[0], wq, t);
    const pair_t* xr = (const pair_t*)a.X[0] + m * a.ldx[0] + 8 * h;
    P::a_load(av, xr, live, 0, Cs, half);
    __syncthreads();
    for (int it = 0;; ++it) {
        int nsrc = src, ncc = cc + 1, noff = off, nCs = Cs;
        const pair_t* nxr = xr;
        if (P::KC * ncc >= Cs) {
            ncc = 0;
            ++nsrc;
            noff = off + Cs;
        }
        const bool more = nsrc < a.nsrc;   // workgroup-uniform
        bool nhalf = false;
        if (more) {
            if (ncc == 0) {
                nCs = a.C[nsrc];
                nxr = (const pair_t*)a.X[nsrc] + m * a.ldx[nsrc] + 8 * h;
            }
            nhalf = P::HALF && nCs - P::KC * ncc < P::KC;
            P::template w_load<NB>(wq, Wt, a.ldw, Ktot, n0, noff + P::KC * ncc, nhalf, t);
            P::a_load(nv, nxr, live, P::KC * ncc, nCs, nhalf);
        }
        if (any) mma_chunk<P, NB>(s_w[it & 1], av, acc, half, r, h);
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
            sum += P::store(Y + ((int64_t)b * a.HW + p) * a.ldy, a.Cout, col, v);
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
// window, k = (ky*3 + kx) * Cin + c, converts them to the policy's operands (X3: split, F16: rounded once),
// and keeps the fragments for every column block; W is [Cout][WORDS][32].
// Lanes r run along xo, so a load's 32 addresses are every other float of one image line.
template <class P>
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
    pair8_t av[4];
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
            P::a_set(av, j, jj, v);
        }
    pair_t* Y = (pair_t*)a.Y;
    for (int nb = 0; nb < a.Cout / 32; ++nb) {
        const int col = 32 * nb + r;
        const pair_t* wr = (const pair_t*)a.Wt + (int64_t)col * (P::WORDS * IMG_STEM_K) + 8 * h;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) acc = P::mma(av, j, wr + 16 * j, wr + IMG_STEM_K + 16 * j, acc);
        const float sh = a.shift[col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + acc_row(i, h);
            if (row >= M) continue;
            float v = acc[i] + sh;
            bad |= f16_unrepresentable(v);
            if (a.relu) v = fmaxf(v, 0.f);
            P::store(Y + (int64_t)row * a.ldy, a.Cout, col, v);
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

// One thread: 8 channels of one pixel, fp32 multiply and add, then one conversion to the row format.  Reads
// come before the writes of the same elements, so Y may be X.
template <class P>
__global__ __launch_bounds__(256) void img_apply_kernel(cmt_img_apply_args a, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int groups = a.C / 8;
    const int64_t row = idx / groups;
    const int c = (int)(idx - row * groups) * 8;
    const int b = (int)(row / a.HW);
    const typename P::Raw8 x = P::load8((const pair_t*)a.X + row * a.ldx + c, a.C);
    const float* g = a.gate + (int64_t)b * a.C + c;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = P::value(x, j) * g[j];
    if (a.R != nullptr) {
        const typename P::Raw8 rr = P::load8((const pair_t*)a.R + row * a.ldr + c, a.C);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += P::value(rr, j);
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) bad |= f16_unrepresentable(v[j]);
    P::write8((pair_t*)a.Y + row * a.ldy, a.C, c, v);
    raise_range_flag(a.range_flag, bad);
}

// One thread: 8 channels of one output pixel.  The window starts inside the map (2 yo <= H - 2) and is
// clipped at the far edges; the maximum starts from the window's first element, never from zero, and the
// winner's words are copied unchanged.
template <class P>
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
    typename P::Raw8 best = P::load8(X + ((int64_t)(b * a.H + 2 * yo) * a.W + 2 * xo) * a.ldx + c, a.C);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int yi = 2 * yo + dy, xi = 2 * xo + dx;
            if ((dy == 0 && dx == 0) || yi >= a.H || xi >= a.W) continue;
            const typename P::Raw8 x = P::load8(X + ((int64_t)(b * a.H + yi) * a.W + xi) * a.ldx + c, a.C);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = P::value(x, j);
                if (v > P::value(best, j) || v != v) P::take(best, x, j);
            }
        }
    P::store8((pair_t*)a.Y + m * a.ldy + c, a.C, best);
}

// ---- host: one validator and launcher per launch kind; `name` is the entry's, WORDS the policy's -----------------
#define IMG_REQUIRE(cond, what) CMT_REQUIRE(cond, std::string(name) + ": " + what)

template <class P>
std::string img_words(const char* what) { return std::string(P::WORDS == 2 ? "2 " : "") + what; }

template <class P>
int img_stem(const char* name, const cmt_img_stem_args* a, void* stream) {
    IMG_REQUIRE(a != nullptr, "null argument struct");
    IMG_REQUIRE(a->X && a->Wt && a->shift && a->Y, "X, Wt, shift and Y must be non-null");
    IMG_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "B, H and W must be positive");
    IMG_REQUIRE(a->Cin >= 1 && a->Cin <= 3, "Cin must be 1, 2 or 3");
    IMG_REQUIRE(a->Cout > 0 && a->Cout % 32 == 0, "Cout must be a positive multiple of 32");
    IMG_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "B*H*W must be below 2^31");
    IMG_REQUIRE(a->x_bstride >= (int64_t)a->Cin * a->H * a->W, "x_bstride below Cin*H*W");
    IMG_REQUIRE(a->ldy >= P::WORDS * (int64_t)a->Cout && (!P::LDY8 || a->ldy % 8 == 0),
                "ldy >= " + img_words<P>("Cout") + (P::LDY8 ? " and % 8 (16-bit words)" : "") + " required");
    IMG_REQUIRE(aligned16(a->Wt) && (((uintptr_t)a->X) & 3) == 0 && (((uintptr_t)a->Y) & 1) == 0,
                "Wt must be 16-byte, X 4-byte and Y 2-byte aligned");
    const int Ho = (a->H - 1) / 2 + 1, Wo = (a->W - 1) / 2 + 1;
    const int64_t M = (int64_t)a->B * Ho * Wo;
    img_stem_kernel<P><<<dim3((unsigned)cdiv64(M, IMG_TM)), 256, 0, (hipStream_t)stream>>>(*a, Ho, Wo, (int)M);
    return cmt_check_launch(name);
}

template <class P, int NB>
void img_conv_launch(const cmt_img_conv_args* a, int Ho, int Wo, int64_t M, hipStream_t s) {
    img_conv3x3_kernel<P, NB><<<dim3((unsigned)cdiv64(M, IMG_TM), (unsigned)(a->Cout / (32 * NB))), 256, 0, s>>>(*a, Ho, Wo, (int)M);
}

template <class P>
int img_conv3x3(const char* name, const cmt_img_conv_args* a, void* stream) {
    IMG_REQUIRE(a != nullptr, "null argument struct");
    IMG_REQUIRE(a->X && a->Wt && a->shift && a->Y, "X, Wt, shift and Y must be non-null");
    IMG_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "B, H and W must be positive");
    IMG_REQUIRE(a->stride == 1 || a->stride == 2, "stride must be 1 or 2");
    IMG_REQUIRE(a->Cin > 0 && a->Cin % 32 == 0, "Cin must be a positive multiple of 32");
    IMG_REQUIRE(a->Cout > 0 && a->Cout % 32 == 0 && a->Cout <= 256, "Cout must be a positive multiple of 32, at most 256");
    IMG_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "B*H*W must be below 2^31");
    IMG_REQUIRE(a->ldx >= P::WORDS * (int64_t)a->Cin && a->ldx % 8 == 0 && a->ldw >= 9 * P::WORDS * (int64_t)a->Cin &&
                    a->ldw % 8 == 0 && a->ldy >= P::WORDS * (int64_t)a->Cout && (!P::LDY8 || a->ldy % 8 == 0),
                "ldx >= " + img_words<P>("Cin") + ", ldw >= " + std::to_string(9 * P::WORDS) + " Cin (both % 8, 16-bit words) and ldy >= " +
                    img_words<P>("Cout") + (P::LDY8 ? " (% 8)" : "") + " required");
    IMG_REQUIRE(aligned16(a->X) && aligned16(a->Wt) && (((uintptr_t)a->Y) & 1) == 0, "X and Wt must be 16-byte aligned");
    const int s = a->stride;
    const int Ho = (a->H - 1) / s + 1, Wo = (a->W - 1) / s + 1;
    const int64_t M = (int64_t)a->B * Ho * Wo;
    hipStream_t st = (hipStream_t)stream;
    // column blocks per workgroup: all of them, unless the row tiles alone leave compute units idle; then the
    // largest divisor of Cout / 32 that gives every unit a workgroup (or 1).  Measured at the V-99-eSE shapes
    // (DESIGN 12): 188 tiles of 192 columns run 1.24 x faster as 3 + 3, 47 tiles of 224 1.8 x faster as 7 x 1.
    const int blocks = a->Cout / 32;
    int nb = a->nb;
    IMG_REQUIRE(nb >= 0 && (nb == 0 || blocks % nb == 0), "nb must be 0 or a divisor of Cout / 32");
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
        case 1: img_conv_launch<P, 1>(a, Ho, Wo, M, st); break;
        case 2: img_conv_launch<P, 2>(a, Ho, Wo, M, st); break;
        case 3: img_conv_launch<P, 3>(a, Ho, Wo, M, st); break;
        case 4: img_conv_launch<P, 4>(a, Ho, Wo, M, st); break;
        case 5: img_conv_launch<P, 5>(a, Ho, Wo, M, st); break;
        case 6: img_conv_launch<P, 6>(a, Ho, Wo, M, st); break;
        case 7: img_conv_launch<P, 7>(a, Ho, Wo, M, st); break;
        default: img_conv_launch<P, 8>(a, Ho, Wo, M, st); break;
    }
    return cmt_check_launch(name);
}

template <class P>
int img_concat1x1(const char* name, const cmt_img_concat_args* a, void* stream) {
    IMG_REQUIRE(a != nullptr, "null argument struct");
    IMG_REQUIRE(a->Wt && a->shift && a->Y, "Wt, shift and Y must be non-null");
    IMG_REQUIRE(a->B > 0 && a->HW > 0, "B and HW must be positive");
    IMG_REQUIRE(a->B <= 65535, "B beyond the grid");
    IMG_REQUIRE(a->nsrc >= 1 && a->nsrc <= CMT_IMG_MAX_SRC, "1 to 8 sources required");
    IMG_REQUIRE(a->Cout > 0 && a->Cout % (32 * IMG_CAT_NB) == 0, "Cout must be a positive multiple of 128");
    IMG_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), "B*HW must be below 2^31");
    int64_t K = 0;
    for (int s = 0; s < a->nsrc; ++s) {
        IMG_REQUIRE(a->X[s] != nullptr && aligned16(a->X[s]), "every source must be non-null and 16-byte aligned");
        IMG_REQUIRE(a->C[s] > 0 && a->C[s] % 32 == 0, "every source width must be a positive multiple of 32");
        IMG_REQUIRE(a->ldx[s] >= P::WORDS * (int64_t)a->C[s] && a->ldx[s] % 8 == 0,
                    "ldx >= " + img_words<P>("C") + " and % 8 (16-bit words) required");
        K += a->C[s];
    }
    IMG_REQUIRE(K < ((int64_t)1 << 24), "K too large");
    IMG_REQUIRE(a->ldw >= P::WORDS * K && a->ldw % 8 == 0 && a->ldy >= P::WORDS * (int64_t)a->Cout && (!P::LDY8 || a->ldy % 8 == 0),
                "ldw >= " + img_words<P>("K") + " (% 8, 16-bit words) and ldy >= " + img_words<P>("Cout") + (P::LDY8 ? " (% 8)" : "") +
                    " required");
    IMG_REQUIRE(aligned16(a->Wt) && (((uintptr_t)a->Y) & 1) == 0 && (((uintptr_t)a->part) & 3) == 0,
                "Wt must be 16-byte aligned, part 4-byte");
    const int tiles = cdiv(a->HW, IMG_TM);
    dim3 grid((unsigned)tiles, (unsigned)(a->Cout / (32 * IMG_CAT_NB)), (unsigned)a->B);
    img_concat_kernel<P><<<grid, 256, 0, (hipStream_t)stream>>>(*a, (int)K, tiles);
    return cmt_check_launch(name);
}

template <class P>
int img_ese_apply(const char* name, const cmt_img_apply_args* a, void* stream) {
    IMG_REQUIRE(a != nullptr, "null argument struct");
    IMG_REQUIRE(a->X && a->gate && a->Y, "X, gate and Y must be non-null");
    IMG_REQUIRE(a->B > 0 && a->HW > 0, "B and HW must be positive");
    IMG_REQUIRE(a->C > 0 && a->C % 8 == 0, "C must be a positive multiple of 8");
    IMG_REQUIRE((int64_t)a->B * a->HW < ((int64_t)1 << 31), "B*HW must be below 2^31");
    IMG_REQUIRE(a->ldx >= P::WORDS * (int64_t)a->C && a->ldx % 8 == 0 && a->ldy >= P::WORDS * (int64_t)a->C && a->ldy % 8 == 0,
                "ldx, ldy >= " + img_words<P>("C") + " and % 8 (16-bit words) required");
    IMG_REQUIRE(aligned16(a->X) && aligned16(a->Y) && aligned16(a->gate), "X, Y and gate must be 16-byte aligned");
    if (a->R != nullptr)
        IMG_REQUIRE(a->ldr >= P::WORDS * (int64_t)a->C && a->ldr % 8 == 0 && aligned16(a->R),
                    "ldr >= " + img_words<P>("C") + ", % 8, and a 16-byte aligned R required");
    const int64_t total = (int64_t)a->B * a->HW * (a->C / 8);
    const int64_t blocks = cdiv64(total, 256);
    IMG_REQUIRE(blocks < ((int64_t)1 << 31), "grid too large");
    img_apply_kernel<P><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, total);
    return cmt_check_launch(name);
}

template <class P>
int img_maxpool(const char* name, const cmt_img_pool_args* a, void* stream) {
    IMG_REQUIRE(a != nullptr, "null argument struct");
    IMG_REQUIRE(a->X && a->Y, "X and Y must be non-null");
    IMG_REQUIRE(a->B > 0 && a->H >= 2 && a->W >= 2, "B positive and H, W >= 2 required");
    IMG_REQUIRE(a->C > 0 && a->C % 8 == 0, "C must be a positive multiple of 8");
    IMG_REQUIRE((int64_t)a->B * a->H * a->W < ((int64_t)1 << 31), "B*H*W must be below 2^31");
    IMG_REQUIRE(a->ldx >= P::WORDS * (int64_t)a->C && a->ldx % 8 == 0 && a->ldy >= P::WORDS * (int64_t)a->C && a->ldy % 8 == 0,
                "ldx, ldy >= " + img_words<P>("C") + " and % 8 (16-bit words) required");
    IMG_REQUIRE(aligned16(a->X) && aligned16(a->Y), "X and Y must be 16-byte aligned");
    const int Ho = (a->H - 2) / 2 + 1, Wo = (a->W - 2) / 2 + 1;
    const int64_t total = (int64_t)a->B * Ho * Wo * (a->C / 8);
    const int64_t blocks = cdiv64(total, 256);
    IMG_REQUIRE(blocks < ((int64_t)1 << 31), "grid too large");
    img_pool_kernel<P><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(*a, Ho, Wo, total);
    return cmt_check_launch(name);
}

}  // namespace

extern "C" int64_t cmt_img_stem_args_size(void) { return (int64_t)sizeof(cmt_img_stem_args); }
extern "C" int64_t cmt_img_conv_args_size(void) { return (int64_t)sizeof(cmt_img_conv_args); }
extern "C" int64_t cmt_img_concat_args_size(void) { return (int64_t)sizeof(cmt_img_concat_args); }
extern "C" int64_t cmt_img_gate_args_size(void) { return (int64_t)sizeof(cmt_img_gate_args); }
extern "C" int64_t cmt_img_apply_args_size(void) { return (int64_t)sizeof(cmt_img_apply_args); }
extern "C" int64_t cmt_img_pool_args_size(void) { return (int64_t)sizeof(cmt_img_pool_args); }
extern "C" int cmt_img_concat_tile_rows(void) { return IMG_TM; }

extern "C" int cmt_img_stem(const cmt_img_stem_args* a, void* s) { return img_stem<X3>("cmt_img_stem", a, s); }
extern "C" int cmt_img_stem_f16(const cmt_img_stem_args* a, void* s) { return img_stem<F16>("cmt_img_stem_f16", a, s); }
extern "C" int cmt_img_conv3x3(const cmt_img_conv_args* a, void* s) { return img_conv3x3<X3>("cmt_img_conv3x3", a, s); }
extern "C" int cmt_img_conv3x3_f16(const cmt_img_conv_args* a, void* s) { return img_conv3x3<F16>("cmt_img_conv3x3_f16", a, s); }
extern "C" int cmt_img_concat1x1(const cmt_img_concat_args* a, void* s) { return img_concat1x1<X3>("cmt_img_concat1x1", a, s); }
extern "C" int cmt_img_concat1x1_f16(const cmt_img_concat_args* a, void* s) {
    return img_concat1x1<F16>("cmt_img_concat1x1_f16", a, s);
}
extern "C" int cmt_img_ese_apply(const cmt_img_apply_args* a, void* s) { return img_ese_apply<X3>("cmt_img_ese_apply", a, s); }
extern "C" int cmt_img_ese_apply_f16(const cmt_img_apply_args* a, void* s) {
    return img_ese_apply<F16>("cmt_img_ese_apply_f16", a, s);
}
extern "C" int cmt_img_maxpool(const cmt_img_pool_args* a, void* s) { return img_maxpool<X3>("cmt_img_maxpool", a, s); }
extern "C" int cmt_img_maxpool_f16(const cmt_img_pool_args* a, void* s) { return img_maxpool<F16>("cmt_img_maxpool_f16", a, s); }

extern "C" int cmt_img_ese_gate(const cmt_img_gate_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_img_ese_gate: null argument struct");
    CMT_REQUIRE(a->part && a->Wfc && a->bias && a->gate, "cmt_img_ese_gate: part, Wfc, bias and gate must be non-null");
    CMT_REQUIRE(a->B > 0 && a->B <= 65535 && a->tiles > 0 && a->HW > 0, "cmt_img_ese_gate: B (<= 65535), tiles and HW must be positive");
    CMT_REQUIRE(a->C > 0 && a->C % 4 == 0 && a->C <= 8192, "cmt_img_ese_gate: C must be a positive multiple of 4, at most 8192");
    dim3 grid((unsigned)cdiv(a->C, IMG_GATE_OB), (unsigned)a->B);
    img_gate_kernel<<<grid, 256, (size_t)a->C * sizeof(float), (hipStream_t)stream>>>(*a);
    return cmt_check_launch("cmt_img_ese_gate");
}
