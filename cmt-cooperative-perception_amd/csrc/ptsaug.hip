// The training-side point and box pipeline of include/cmt_hip.h on the device:
//   cmt_points_in_boxes: the point-in-rotated-box test (points_in_rbbox) -> lowest containing box per point,
//                        points per box;
//   cmt_pts_augment:     object paste (remove_points_in_boxes + concatenation), GlobalRotScaleTrans, flips, the
//                        range filter and the shuffle of one cloud as an order-preserving stream compaction over
//                        the visited sequence;
//   cmt_boxes_augment:   the same parameters on the annotations, with ObjectRangeFilter, ObjectNameFilter,
//                        limit_yaw and the gravity-centre layout, in one workgroup.
//
// cmt_pts_augment has the structure of ptsprep.hip: the count and the scatter launch of wave_ops.h's compaction
// (compact_count, compact_scatter) over tiles of AUG_T consecutive slots, with aug_slot as the row function of both.
// The boxes are staged in LDS as centre, half extents and one sinf / cosf pair each: both launches of
// cmt_pts_augment compute them with the same instructions, so a point near a face falls on the same side in both.
// Contraction is off for the row functions (and for the file, see the Makefile): the contract's products and
// sums are separate roundings.  The tile constants and aug_stage / aug_inside are aug_inside.h, which gtdb.hip
// includes too: its extraction puts a point near a face on the same side as the calls here.
#include "aug_inside.h"

// rotation, scale, translation and flips on v[0..2]
__device__ __forceinline__ void aug_xform_point(const cmt_aug_xform& t, float* v) {
#pragma clang fp contract(off)
    if (t.has_rot) {
        const float a = v[0], b = v[1], d = v[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float m0 = a * t.rot32[3 * k], m1 = b * t.rot32[3 * k + 1], m2 = d * t.rot32[3 * k + 2];
            v[k] = (m0 + m1) + m2;
        }
    }
    if (t.has_scale) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] * t.scale;
    }
    if (t.has_trans) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] + t.trans32[k];
    }
    if (t.flip_h) v[1] = -v[1];
    if (t.flip_v) v[0] = -v[0];
}

// ---- cmt_points_in_boxes ------------------------------------------------------------------------------------
struct pib_p {
    const float* pts;
    const int* count_in;
    const float* boxes;
    int* box_of_point;
    int* count_per_box;
    unsigned N;
    int M, F, D;
};

__global__ __launch_bounds__(AUG_THREADS) void pib_kernel(pib_p p) {
    __shared__ aug_box bx[PIB_CB];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned t0 = blockIdx.x * (unsigned)AUG_T;
    const unsigned cnt = (unsigned)clamp_count(p.count_in, p.N);
    float x[AUG_R], y[AUG_R], z[AUG_R];
    int first[AUG_R];
#pragma unroll
    for (int r = 0; r < AUG_R; ++r) {
        const unsigned i = t0 + (unsigned)((r * 4 + w) * 64 + lane);
        x[r] = y[r] = z[r] = __builtin_nanf("");   // a row that does not exist is inside nothing
        first[r] = -1;
        if (i < cnt) {
            const float* q = p.pts + (int64_t)i * p.F;
            x[r] = q[0], y[r] = q[1], z[r] = q[2];
        }
    }
    for (int b0 = 0; b0 < p.M; b0 += PIB_CB) {
        const int nb = p.M - b0 < PIB_CB ? p.M - b0 : PIB_CB;
        __syncthreads();   // the previous chunk has been read
        if ((int)threadIdx.x < nb) bx[threadIdx.x] = aug_stage(p.boxes + (int64_t)(b0 + (int)threadIdx.x) * p.D);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const aug_box box = bx[b];
            int hits = 0;
#pragma unroll
            for (int r = 0; r < AUG_R; ++r) {
                const bool in = aug_inside(box, x[r], y[r], z[r]);
                if (in && first[r] < 0) first[r] = b0 + b;
                hits += __popcll(__ballot(in));
            }
            if (p.count_per_box && hits > 0 && lane == 0) atomicAdd(p.count_per_box + b0 + b, hits);
        }
    }
    if (p.box_of_point) {
#pragma unroll
        for (int r = 0; r < AUG_R; ++r) {
            const unsigned i = t0 + (unsigned)((r * 4 + w) * 64 + lane);
            if (i < p.N) p.box_of_point[i] = first[r];
        }
    }
}

// ---- cmt_pts_augment ----------------------------------------------------------------------------------------
struct aug_p {
    const float* src;
    const float* paste;
    const float* boxes;
    const int* count_in;
    const int* order;
    float* dst;
    int* count;
    int* tile_cnt;       // the workspace: kept rows of each tile
    unsigned n_src, n_paste, n_in;
    int tiles, F, K, paste_first;
    cmt_aug_xform xf;
};

__device__ __forceinline__ void aug_stage_all(const aug_p& p, aug_box* bx) {
    if ((int)threadIdx.x < p.K) bx[threadIdx.x] = aug_stage(p.boxes + (int64_t)threadIdx.x * 7);
    __syncthreads();
}

// slot j: the keep predicate and, in o[0 .. F), the output row.  Both kernels call this.
__device__ __forceinline__ bool aug_slot(const aug_p& p, const aug_box* bx, unsigned cnt, unsigned j, float (&o)[8]) {
#pragma clang fp contract(off)
    if (j >= p.n_in) return false;
    const int oi = p.order ? p.order[j] : (int)j;
    if (oi < 0 || (unsigned)oi >= p.n_in) return false;
    const unsigned i = (unsigned)oi;
    bool pasted;
    unsigned r;
    if (p.paste_first) {
        pasted = i < p.n_paste;
        r = pasted ? i : i - p.n_paste;
    } else {
        pasted = i >= p.n_src;
        r = pasted ? i - p.n_src : i;
    }
    if (!pasted && r >= cnt) return false;
    const float* q = (pasted ? p.paste : p.src) + (int64_t)r * p.F;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < p.F) o[k] = q[k];
    bool keep = true;
    if (!pasted) {
        for (int b = 0; b < p.K; ++b) keep = keep && !aug_inside(bx[b], o[0], o[1], o[2]);
    }
    aug_xform_point(p.xf, o);
    if (p.xf.has_range) {
#pragma unroll
        for (int k = 0; k < 3; ++k) keep = keep && o[k] > p.xf.range[k] && o[k] < p.xf.range[3 + k];
    }
    return keep;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_count_kernel(aug_p p) {
    __shared__ aug_box bx[CMT_AUG_MAX_BOXES];
    aug_stage_all(p, bx);
    const unsigned cnt = (unsigned)clamp_count(p.count_in, p.n_src);
    compact_count(p.tile_cnt, [&](unsigned j, float (&o)[8]) { return aug_slot(p, bx, cnt, j, o); });
}

__global__ __launch_bounds__(AUG_THREADS) void aug_scatter_kernel(aug_p p) {
    __shared__ aug_box bx[CMT_AUG_MAX_BOXES];
    aug_stage_all(p, bx);
    const unsigned cnt = (unsigned)clamp_count(p.count_in, p.n_src);
    compact_scatter(p.tile_cnt, p.tiles, p.dst, p.count, p.n_in, p.F,
                    [&](unsigned j, float (&o)[8]) { return aug_slot(p, bx, cnt, j, o); });
}

// ---- cmt_boxes_augment --------------------------------------------------------------------------------------
struct box_p {
    const float* boxes;
    const long long* labels;
    float* out_boxes;
    long long* out_labels;
    int* count;
    int n, D, num_classes, gravity;
    cmt_aug_xform xf;
};

__device__ __forceinline__ bool aug_box_eval(const box_p& p, float (&b)[9], long long label) {
#pragma clang fp contract(off)
    const cmt_aug_xform& t = p.xf;
    if (t.has_rot) {
        const float vx = b[7], vy = b[8];
        const float a0 = vx * t.rot32[0], a1 = vy * t.rot32[1], a3 = vx * t.rot32[3], a4 = vy * t.rot32[4];
        b[7] = a0 + a1;
        b[8] = a3 + a4;
        b[6] = b[6] + t.angle32;
    }
    float yaw = b[6];
    // the centre like a point; its flips are the box's column 1 / column 0 sign changes
    aug_xform_point(t, b);
    if (t.has_scale) {
#pragma unroll
        for (int k = 3; k < 9; ++k)
            if (k != 6) b[k] = b[k] * t.scale;
    }
    if (t.flip_h) {
        b[8] = -b[8];
        yaw = -yaw;
    }
    if (t.flip_v) {
        b[7] = -b[7];
        yaw = -yaw + 3.14159274101257324f;
    }
    bool keep = true;
    if (t.has_range) keep = b[0] > t.range[0] && b[1] > t.range[1] && b[0] < t.range[3] && b[1] < t.range[4];
    keep = keep && label >= 0 && label < (long long)p.num_classes;
    const float P = 6.28318548202636719f;
    const float turns = floorf(yaw / P + 0.5f);
    b[6] = yaw - turns * P;
    if (p.gravity) b[2] = b[2] + b[5] * 0.5f;
    return keep;
}

__global__ __launch_bounds__(AUG_THREADS) void boxes_augment_kernel(box_p p) {
    __shared__ int tab[4];
    int base = 0;   // kept boxes in front of this pass, the same in every thread
    for (int c0 = 0; c0 < p.n; c0 += AUG_THREADS) {
        const int i = c0 + (int)threadIdx.x;
        float b[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) b[k] = 0.f;
        long long label = -1;
        bool keep[1] = {false};
        if (i < p.n) {
            const float* q = p.boxes + (int64_t)i * p.D;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (k < p.D) b[k] = q[k];
            label = p.labels[i];
            keep[0] = aug_box_eval(p, b, label);
        }
        int rank[1];
        const int tot = tile_rank<1>(keep, rank, tab);
        if (keep[0]) {
            const int g = base + rank[0];   // <= i
            float* q = p.out_boxes + (int64_t)g * p.D;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (k < p.D) q[k] = b[k];
            p.out_labels[g] = label;
        }
        base += tot;
    }
    for (int i = base + (int)threadIdx.x; i < p.n; i += AUG_THREADS) {
        unsigned* q = (unsigned*)p.out_boxes + (int64_t)i * p.D;
        for (int k = 0; k < p.D; ++k) q[k] = QNAN32;
        p.out_labels[i] = -1;
    }
    if (threadIdx.x == 0) *p.count = base;
}

// ---- host ---------------------------------------------------------------------------------------------------
static const char* aug_xform_error(const cmt_aug_xform& t) {
    if (t.has_rot) {
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(t.rot32[k])) return "non-finite rotation";
        if (!std::isfinite(t.angle32)) return "non-finite rotation angle";
    }
    if (t.has_scale && !std::isfinite(t.scale)) return "non-finite scale";
    if (t.has_trans)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(t.trans32[k])) return "non-finite translation";
    if (t.has_range) {
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(t.range[k])) return "non-finite range";
        for (int k = 0; k < 3; ++k)
            if (!(t.range[k] < t.range[3 + k])) return "range min must be below max";
    }
    return nullptr;
}

extern "C" int64_t cmt_points_in_boxes_args_size(void) { return (int64_t)sizeof(cmt_points_in_boxes_args); }
extern "C" int64_t cmt_pts_augment_args_size(void) { return (int64_t)sizeof(cmt_pts_augment_args); }
extern "C" int64_t cmt_boxes_augment_args_size(void) { return (int64_t)sizeof(cmt_boxes_augment_args); }
extern "C" int cmt_points_in_boxes_chunk(void) { return PIB_CB; }
extern "C" int cmt_pts_augment_tile_rows(void) { return AUG_T; }

extern "C" int64_t cmt_pts_augment_workspace_bytes(int64_t n_in) {
    if (n_in <= 0) return 0;
    return cdiv64(n_in, AUG_T) * (int64_t)sizeof(int);
}

extern "C" int cmt_points_in_boxes(const cmt_points_in_boxes_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_points_in_boxes: null argument struct");
    CMT_REQUIRE(a->N >= 0 && a->N < ((int64_t)1 << 31), "cmt_points_in_boxes: N must be in [0, 2^31)");
    CMT_REQUIRE(a->M >= 0 && a->M < (1 << 24), "cmt_points_in_boxes: M must be in [0, 2^24)");
    CMT_REQUIRE(a->F >= 3 && a->F <= 8, "cmt_points_in_boxes: F must be 3..8");
    CMT_REQUIRE(a->D == 7 || a->D == 9, "cmt_points_in_boxes: D must be 7 or 9");
    if (a->N > 0) CMT_REQUIRE(ptr_aligned(a->points, 4), "cmt_points_in_boxes: points must be non-null and 4-byte aligned");
    if (a->M > 0) CMT_REQUIRE(ptr_aligned(a->boxes, 4), "cmt_points_in_boxes: boxes must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->count_in, 4) && ptr_aligned_or_null(a->box_of_point, 4) && ptr_aligned_or_null(a->count_per_box, 4),
                "cmt_points_in_boxes: count_in, box_of_point and count_per_box must be 4-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    pib_p p;
    p.pts = (const float*)a->points;
    p.count_in = a->count_in;
    p.boxes = (const float*)a->boxes;
    p.box_of_point = a->box_of_point;
    p.count_per_box = a->M > 0 ? a->count_per_box : nullptr;
    p.N = (unsigned)a->N;
    p.M = a->M, p.F = a->F, p.D = a->D;
    if (p.count_per_box && hipMemsetAsync(p.count_per_box, 0, (size_t)a->M * sizeof(int), st) != hipSuccess)
        return cmt_check_launch("cmt_points_in_boxes");
    const int64_t tiles = cdiv64(a->N, AUG_T);
    if (tiles > 0 && (p.box_of_point || p.count_per_box)) pib_kernel<<<dim3((unsigned)tiles), AUG_THREADS, 0, st>>>(p);
    return cmt_check_launch("cmt_points_in_boxes");
}

extern "C" int cmt_pts_augment(const cmt_pts_augment_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_pts_augment: null argument struct");
    CMT_REQUIRE(a->F >= 3 && a->F <= 8, "cmt_pts_augment: F must be 3..8");
    CMT_REQUIRE(a->K >= 0 && a->K <= CMT_AUG_MAX_BOXES, "cmt_pts_augment: K must be 0..128");
    CMT_REQUIRE(a->n_src >= 0 && a->n_paste >= 0, "cmt_pts_augment: n_src and n_paste must not be negative");
    CMT_REQUIRE(a->n_src < ((int64_t)1 << 31) && a->n_paste < ((int64_t)1 << 31) && a->n_src + a->n_paste < ((int64_t)1 << 31),
                "cmt_pts_augment: n_src + n_paste must be below 2^31");
    CMT_REQUIRE(a->shift_height == 0, "cmt_pts_augment: shift_height is not built");
    if (const char* e = aug_xform_error(a->xf)) return cmt_fail(CMT_EINVAL, std::string("cmt_pts_augment: ") + e);
    const int64_t n_in = a->n_src + a->n_paste;
    CMT_REQUIRE(ptr_aligned(a->count, 4), "cmt_pts_augment: count must be non-null and 4-byte aligned");
    CMT_REQUIRE(ptr_aligned_or_null(a->count_in, 4) && ptr_aligned_or_null(a->order, 4), "cmt_pts_augment: count_in and order must be 4-byte aligned");
    if (a->n_src > 0) CMT_REQUIRE(ptr_aligned(a->src, 4), "cmt_pts_augment: src must be non-null and 4-byte aligned");
    if (a->n_paste > 0) CMT_REQUIRE(ptr_aligned(a->paste, 4), "cmt_pts_augment: paste must be non-null and 4-byte aligned");
    if (a->K > 0) CMT_REQUIRE(ptr_aligned(a->paste_boxes, 4), "cmt_pts_augment: paste_boxes must be non-null and 4-byte aligned");
    if (n_in > 0) {
        CMT_REQUIRE(ptr_aligned(a->dst, 4), "cmt_pts_augment: dst must be non-null and 4-byte aligned");
        CMT_REQUIRE(ptr_aligned(a->workspace, 4), "cmt_pts_augment: workspace must be non-null and 4-byte aligned");
        CMT_REQUIRE(a->workspace_bytes >= cmt_pts_augment_workspace_bytes(n_in),
                    "cmt_pts_augment: workspace below cmt_pts_augment_workspace_bytes(n_in)");
    }
    aug_p p;
    p.src = (const float*)a->src;
    p.paste = (const float*)a->paste;
    p.boxes = (const float*)a->paste_boxes;
    p.count_in = a->count_in;
    p.order = a->order;
    p.dst = (float*)a->dst;
    p.count = a->count;
    p.tile_cnt = (int*)a->workspace;
    p.n_src = (unsigned)a->n_src, p.n_paste = (unsigned)a->n_paste, p.n_in = (unsigned)n_in;
    p.tiles = (int)cdiv64(n_in, AUG_T);
    p.F = a->F, p.K = a->K, p.paste_first = a->paste_first ? 1 : 0;
    p.xf = a->xf;
    const hipStream_t st = (hipStream_t)stream;
    if (p.tiles > 0) aug_count_kernel<<<dim3((unsigned)p.tiles), AUG_THREADS, 0, st>>>(p);
    // with no rows one workgroup still writes count = 0
    aug_scatter_kernel<<<dim3((unsigned)(p.tiles > 0 ? p.tiles : 1)), AUG_THREADS, 0, st>>>(p);
    return cmt_check_launch("cmt_pts_augment");
}

extern "C" int cmt_boxes_augment(const cmt_boxes_augment_args* a, void* stream) {
    CMT_REQUIRE(a != nullptr, "cmt_boxes_augment: null argument struct");
    CMT_REQUIRE(a->n >= 0 && a->n <= CMT_AUG_MAX_ANN, "cmt_boxes_augment: n must be 0..65536");
    CMT_REQUIRE(a->D == 7 || a->D == 9, "cmt_boxes_augment: D must be 7 or 9");
    CMT_REQUIRE(a->num_classes >= 0, "cmt_boxes_augment: num_classes must not be negative");
    if (const char* e = aug_xform_error(a->xf)) return cmt_fail(CMT_EINVAL, std::string("cmt_boxes_augment: ") + e);
    CMT_REQUIRE(ptr_aligned(a->count, 4), "cmt_boxes_augment: count must be non-null and 4-byte aligned");
    if (a->n > 0) {
        CMT_REQUIRE(ptr_aligned(a->boxes, 4) && ptr_aligned(a->out_boxes, 4),
                    "cmt_boxes_augment: boxes and out_boxes must be non-null and 4-byte aligned");
        CMT_REQUIRE(ptr_aligned(a->labels, 8) && ptr_aligned(a->out_labels, 8),
                    "cmt_boxes_augment: labels and out_labels must be non-null and 8-byte aligned");
    }
    box_p p;
    p.boxes = (const float*)a->boxes;
    p.labels = (const long long*)a->labels;
    p.out_boxes = (float*)a->out_boxes;
    p.out_labels = (long long*)a->out_labels;
    p.count = a->count;
    p.n = a->n, p.D = a->D, p.num_classes = a->num_classes, p.gravity = a->gravity ? 1 : 0;
    p.xf = a->xf;
    boxes_augment_kernel<<<dim3(1), AUG_THREADS, 0, (hipStream_t)stream>>>(p);
    return cmt_check_launch("cmt_boxes_augment");
}
